"""The extractor's kernels between the convs (cwt_debug_backbone_op), one at a time, against
float64 torch on the CPU, in every activation layout (fp32 NHWC, the S-layout, bf16 NHWC): the
stem's first conv, the max-pool, the PPM's adaptive pooling, its two small-M GEMMs in both
forms, the training-mode BatchNorm and the bf16 widen.  Whole extractions reach these only
with post-ReLU inputs, odd square maps and one GEMM form per batch size; here the data is
chosen so that a wrong padding value, a missing floor, a wrong stride or a wrong form shows."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dropout_ref import dropout_scale

pytestmark = pytest.mark.gpu

ACT_F32, ACT_SPLIT, ACT_BF16 = 0, 1, 2
LAYOUTS = [ACT_F32, ACT_SPLIT, ACT_BF16]
LAYOUT_IDS = ["f32", "split", "bf16"]
BINS = (1, 2, 3, 6)
TOL_F32 = 1e-5  # the suite's exact-fp32 bar (test_gpu_conv.TOLS[0], test_gpu_conv_s.TOL_F32D)


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def op(opcode, bufs, ia, fa=()):
    from few_shot_seg_cwt_amd import _lib
    b = (C.c_void_p * len(bufs))(*[None if t is None else t.data_ptr() for t in bufs])
    i = (C.c_int64 * len(ia))(*ia)
    f = (C.c_float * len(fa))(*fa) if fa else None
    _lib.check(_lib.lib().cwt_debug_backbone_op(_lib.ctx(0), opcode, b, i, f, _lib.stream_ptr()), "backbone_op")
    torch.cuda.synchronize()


def split(t):
    """fp32 [P][C] (device) -> S-layout bf16 [P][C/32][64] (as tests/test_gpu_conv_s.py)"""
    from few_shot_seg_cwt_amd import _lib as L
    P, Cc = t.shape
    out = torch.empty(P * Cc * 2, dtype=torch.bfloat16, device=t.device)
    L.check(L.lib().cwt_debug_split_act(L.ctx(0), L.ptr(t), P, Cc, Cc, L.ptr(out), L.stream_ptr()), "split")
    return out


def unsplit(s, P, Cc):
    from few_shot_seg_cwt_amd import _lib as L
    out = torch.empty(P, Cc, device=s.device)
    L.check(L.lib().cwt_debug_unsplit_act(L.ctx(0), L.ptr(s), P, Cc, L.ptr(out), Cc, L.stream_ptr()), "unsplit")
    torch.cuda.synchronize()
    return out


def hi_lo(s, P, Cc):
    """The two bf16 planes of an S-layout buffer, each as [P][C]."""
    v = s.view(P, Cc // 32, 2, 32)
    return v[:, :, 0].reshape(P, Cc), v[:, :, 1].reshape(P, Cc)


def bf16r(t):
    return t.to(torch.bfloat16).to(t.dtype)


def down2(x):
    return (x - 1) // 2 + 1


# --------------------------------------------------------------------------------------------
# stem conv1
# --------------------------------------------------------------------------------------------
_stem_cache = {}


def _stem(dev, N, S, relu):
    """Inputs, the float64 reference [N*Ho*Ho][64] and the ACT_F32 kernel output, once per case."""
    key = (N, S, relu)
    if key not in _stem_cache:
        g = torch.Generator().manual_seed(1000 + 10 * (N * 100 + S) + relu)
        img = torch.randn(N, 3, S, S, generator=g)
        w = torch.randn(64, 3, 3, 3, generator=g) * 0.2
        scale = torch.rand(64, generator=g) + 0.5
        shift = torch.randn(64, generator=g) * 0.5
        y = F.conv2d(img.double(), w.double(), None, 2, 1)
        y = y * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
        if relu:
            y = y.clamp_min(0)
        ref = y.permute(0, 2, 3, 1).reshape(-1, 64)
        d = dict(img=img.to(dev), w=w.reshape(64, 27).t().contiguous().to(dev), scale=scale.to(dev),
                 shift=shift.to(dev))
        out = torch.full((ref.shape[0], 64), float("nan"), device=dev)
        op(0, [d["img"], d["w"], d["scale"], d["shift"], out], [N, S, ACT_F32, relu])
        _stem_cache[key] = (d, ref, out)
    return _stem_cache[key]


STEM_CASES = [(1, 9), (3, 9), (2, 33)]  # 25 pixels: a partial 16-pixel group; 75: groups straddle images; Ho = 17


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("N,S", STEM_CASES)
def test_stem_conv1_f32(dev, N, S, relu):
    _, ref, out = _stem(dev, N, S, relu)
    assert ref.shape[0] == N * down2(S) ** 2
    e = rel(out, ref)
    print(f"stem conv1 N={N} S={S} relu={relu}: rel {e:.3e}")
    assert e < TOL_F32
    neg = float((ref < 0).double().mean())
    if relu:
        assert float(out.min()) == 0.0 and 0.3 < float((ref == 0).double().mean()) < 0.7
    else:  # the raw conv of the training-mode BN pass: negative outputs survive
        assert 0.3 < neg < 0.7 and float(out.min()) < -0.5


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("N,S", STEM_CASES)
def test_stem_conv1_bf16(dev, N, S, relu):
    """The three store forms run one f32 MFMA chain: the bf16 output is the rounded fp32 output."""
    d, _, out_f32 = _stem(dev, N, S, relu)
    out = torch.full((out_f32.shape[0], 64), float("nan"), dtype=torch.bfloat16, device=dev)
    op(0, [d["img"], d["w"], d["scale"], d["shift"], out], [N, S, ACT_BF16, relu])
    assert torch.equal(out, out_f32.to(torch.bfloat16))


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("N,S", STEM_CASES)
def test_stem_conv1_split(dev, N, S, relu):
    d, _, out_f32 = _stem(dev, N, S, relu)
    P = out_f32.shape[0]
    out = torch.full((P * 128,), float("nan"), dtype=torch.bfloat16, device=dev)
    op(0, [d["img"], d["w"], d["scale"], d["shift"], out], [N, S, ACT_SPLIT, relu])
    hi, lo = hi_lo(out, P, 64)
    assert torch.equal(hi, out_f32.to(torch.bfloat16))
    s = hi.double() + lo.double()
    assert bool(((s - out_f32.double()).abs() <= 2.0 ** -16 * out_f32.double().abs()).all())
    assert torch.equal(unsplit(out, P, 64).double(), s)


# --------------------------------------------------------------------------------------------
# max-pool 3x3 s2 p1
# --------------------------------------------------------------------------------------------
# from the third on: even extents and H != W (the product only sends odd squares).  Wo is odd in
# the first four (the pair kernel's last pair is half empty) and even in the last (W = 8 -> Wo = 4:
# its last pair is whole and the right-hand window ends on the last input column)
POOL_CASES = [(1, 5, 5, 32), (2, 17, 17, 128), (1, 6, 9, 64), (3, 9, 6, 128), (2, 7, 8, 32)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("N,H,W,Cc", POOL_CASES)
def test_maxpool(dev, N, H, W, Cc, layout):
    """Bit-exact: a maximum of representable values is representable.  The input is N(-3, 1),
    nearly all negative, so any padding value but -inf wins the border windows."""
    g = torch.Generator().manual_seed(2000 + H * 100 + W)
    x = torch.randn(N, H, W, Cc, generator=g) - 3.0
    Ho, Wo = down2(H), down2(W)
    P, Po = N * H * W, N * Ho * Wo
    if layout == ACT_SPLIT:  # fp32 values with a non-zero lo part
        xs = split(x.reshape(P, Cc).to(dev))
        assert float(hi_lo(xs, P, Cc)[1].float().abs().max()) > 0
        xin = unsplit(xs, P, Cc).cpu().reshape(N, H, W, Cc)
        out = torch.full((Po * Cc * 2,), float("nan"), dtype=torch.bfloat16, device=dev)
        op(1, [xs, out], [N, H, W, Cc, layout])
        got = unsplit(out, Po, Cc).cpu()
    else:
        xin = bf16r(x)
        dt = torch.float32 if layout == ACT_F32 else torch.bfloat16
        xd = xin.to(dt).to(dev).contiguous()
        out = torch.full((Po, Cc), float("nan"), dtype=dt, device=dev)
        op(1, [xd, out], [N, H, W, Cc, layout])
        got = out.float().cpu()
    ref = F.max_pool2d(xin.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).reshape(Po, Cc)
    assert float((ref < 0).float().mean()) > 0.9  # a zero padding would win nearly every border window
    assert torch.equal(got, ref)


# --------------------------------------------------------------------------------------------
# PPM adaptive average pooling
# --------------------------------------------------------------------------------------------
def make_segs(n):
    """Lengths of the elementary segments of backbone.hip's make_segs over the four bins."""
    b = set()
    for k in BINS:
        for i in range(k):
            b.add(i * n // k)
            b.add(((i + 1) * n + k - 1) // k)
    b = sorted(b)
    return [b[i + 1] - b[i] for i in range(len(b) - 1)]


def test_ppm_segment_cases():
    """What the chosen sides exercise (host only).  21 has no segment longer than 3; 54 is the
    smallest side with one longer than 8 (ppm_rowseg8_kernel's second u0 pass), 6 segments of 9."""
    assert max(make_segs(21)) == 3 and all(max(make_segs(h)) <= 8 for h in range(1, 54))
    assert make_segs(54) == [9] * 6
    assert all(len(make_segs(h)) <= 16 for h in (5, 9, 13, 21, 54))
    assert len(make_segs(5)) == 5 and 13 % 2 and 13 % 3 and 13 % 6


PPM_CASES = [(N, h, h) for h in (5, 9, 13, 21, 54) for N in (1, 3)] + [(1, 9, 13)]
_ppm_cache = {}


def _ppm(dev, N, h, w):
    """bf16-exact input [N][h][w][2048], the float64 reference (bin-major [50 N][2048], as
    ppm_cell_kernel writes it) and the ACT_F32 kernel result on it."""
    key = (N, h, w)
    if key not in _ppm_cache:
        g = torch.Generator().manual_seed(3000 + N * 10000 + h * 100 + w)
        x = bf16r(torch.randn(N, h, w, 2048, generator=g))
        xd = x.to(dev)
        out = torch.full((50 * N, 2048), float("nan"), device=dev)
        op(2, [xd, out], [N, h, w, 2048, ACT_F32])
        _ppm_cache.clear()  # one case's tensors at a time
        _ppm_cache[key] = (x, _ppm_ref(x), out.cpu())
    return _ppm_cache[key]


def _ppm_ref(x):
    N = x.shape[0]
    xc = x.double().permute(0, 3, 1, 2)
    return torch.cat([F.adaptive_avg_pool2d(xc, b).permute(0, 2, 3, 1).reshape(N * b * b, -1) for b in BINS])


def _ppm_check(got, ref):
    got = got.double().cpu()
    e = float((got - ref).abs().max() / ref.abs().max())
    print(f"ppm pooling: rel {e:.3e}")
    assert e < 1e-6
    assert bool(((got - ref).abs() <= 1e-6 * ref.abs().max()).all())


@pytest.mark.parametrize("N,h,w", PPM_CASES)
def test_ppm_pool_f32(dev, N, h, w):
    g = torch.Generator().manual_seed(3500 + N * 10000 + h * 100 + w)
    x = torch.randn(N, h, w, 2048, generator=g)  # full fp32 mantissas
    out = torch.full((50 * N, 2048), float("nan"), device=dev)
    op(2, [x.to(dev), out], [N, h, w, 2048, ACT_F32])
    _ppm_check(out, _ppm_ref(x))


@pytest.mark.parametrize("N,h,w", [(3, 13, 13), (1, 9, 13)])
def test_ppm_pool_f32_stride(dev, N, h, w):
    """Pixel stride 2112 > C, the padding poisoned: same bits as the dense map."""
    x, ref, dense = _ppm(dev, N, h, w)
    xp = torch.full((N, h, w, 2112), float("nan"))
    xp[..., :2048] = x
    out = torch.full((50 * N, 2048), float("nan"), device=dev)
    op(2, [xp.to(dev), out], [N, h, w, 2112, ACT_F32])
    _ppm_check(out, ref)
    assert torch.equal(out.cpu(), dense)


@pytest.mark.parametrize("layout", [ACT_SPLIT, ACT_BF16], ids=["split", "bf16"])
@pytest.mark.parametrize("N,h,w", PPM_CASES)
def test_ppm_pool_16bit(dev, N, h, w, layout):
    """The 8-channel kernel on bf16-exact input: the float64 bar, and bitwise the fp32 kernel's
    result on the same values (backbone.hip: the same summation order)."""
    x, ref, out_f32 = _ppm(dev, N, h, w)
    P = N * h * w
    xd = x.reshape(P, 2048).to(dev)
    xs = split(xd) if layout == ACT_SPLIT else xd.to(torch.bfloat16)
    out = torch.full((50 * N, 2048), float("nan"), device=dev)
    op(2, [xs, out], [N, h, w, 2048, layout])
    _ppm_check(out, ref)
    assert torch.equal(out.cpu(), out_f32)


# --------------------------------------------------------------------------------------------
# PPM GEMMs
# --------------------------------------------------------------------------------------------
GEMMS = {"conv": (2048, 512, 32, True), "fold": (512, 4608, 64, False)}  # K, N, run_extract's K chunk, BN + ReLU
_gemm_cache = {}


def _gemm(dev, which, n):
    """Inputs, float64 reference and the outputs of the explicit forms 0 (MFMA) and 1 (split-K)."""
    key = (which, n)
    if key not in _gemm_cache:
        K, Nn, kc, bn = GEMMS[which]
        M = [n * b * b for b in BINS]
        g = torch.Generator().manual_seed(4000 + K + n)
        A = torch.randn(sum(M), K, generator=g)
        Bt = [torch.randn(K, Nn, generator=g) * K ** -0.5 for _ in range(4)]
        sc = [torch.rand(Nn, generator=g) + 0.5 for _ in range(4)] if bn else [None] * 4
        sh = [torch.randn(Nn, generator=g) * 0.5 for _ in range(4)] if bn else [None] * 4
        refs, r0 = [], 0
        for q in range(4):
            y = A[r0:r0 + M[q]].double() @ Bt[q].double()
            if bn:
                y = (y * sc[q].double() + sh[q].double()).clamp_min(0)
            refs.append(y)
            r0 += M[q]
        mv = lambda ts: [None if t is None else t.to(dev) for t in ts]  # noqa: E731
        bufs = [A.to(dev)] + mv(Bt) + mv(sc) + mv(sh)

        def run(form):
            out = torch.full((sum(M), Nn), float("nan"), device=dev)
            op(3, bufs + [out], M + [Nn, K, kc, form])
            return out.cpu()
        _gemm_cache.clear()
        _gemm_cache[key] = (torch.cat(refs), run, {0: run(0), 1: run(1)})
    return _gemm_cache[key]


@pytest.mark.parametrize("n", [1, 4, 5])
@pytest.mark.parametrize("which", ["conv", "fold"])
def test_ppm_gemm_forms(dev, which, n):
    """Both forms against float64 (fp32 sums over K <= 2048), and the automatic choice: the MFMA
    form up to 200 cells (n = 4), the split-K form from 250 (n = 5), bitwise."""
    ref, run, outs = _gemm(dev, which, n)
    for form, out in outs.items():
        e = rel(out, ref)
        print(f"ppm gemm {which} n={n} form {form}: rel {e:.3e}")
        assert e < TOL_F32, form
    if GEMMS[which][3]:
        assert 0.3 < float((ref == 0).double().mean()) < 0.7  # the ReLU clips about half
    auto = run(-1)
    assert torch.equal(auto, outs[0 if 50 * n <= 200 else 1])
    assert not torch.equal(outs[0], outs[1])  # the two forms sum in different orders


# --------------------------------------------------------------------------------------------
# training-mode BatchNorm
# --------------------------------------------------------------------------------------------
EPS, MOM = 1e-5, 0.1
# (M, C, rows_per_image, drop_p): the minimum; layer4 at S = 33; one row into a second stats
# block; three 9 x 9 images with Dropout2d
BN_CASES = [(2, 64, 2, 0.0), (50, 2048, 25, 0.0), (257, 128, 257, 0.0), (3 * 81, 512, 81, 0.5)]
DROP_SEED = 12345


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("M,Cc,rpi,drop_p", BN_CASES)
def test_bn_train(dev, M, Cc, rpi, drop_p, layout, with_res, relu):
    g = torch.Generator().manual_seed(5000 + M + Cc)
    mu = torch.rand(Cc, generator=g) * 8 - 4
    y = torch.randn(M, Cc, generator=g) + mu
    res = torch.randn(M, Cc, generator=g) if with_res else None
    bn = torch.stack([torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.5,
                      torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5])
    bn_d = bn.to(dev).contiguous()
    scale = torch.full((Cc,), float("nan"), device=dev)
    shift = torch.full((Cc,), float("nan"), device=dev)

    def store(t):  # -> (device buffer in the layout, the values it holds)
        if t is None:
            return None, None
        if layout == ACT_F32:
            return t.to(dev).contiguous(), t
        if layout == ACT_BF16:
            b = t.to(torch.bfloat16).to(dev).contiguous()
            return b, b.float().cpu()
        s = split(t.to(dev).contiguous())
        return s, unsplit(s, M, Cc).cpu()
    yb, yv = store(y)
    rb, rv_ = store(res)
    op(4, [yb, rb, bn_d, scale, shift], [M, Cc, layout, Cc, Cc, relu, rpi, DROP_SEED], [EPS, MOM, drop_p])
    got = (yb if layout == ACT_F32 else yb.float() if layout == ACT_BF16 else unsplit(yb, M, Cc)).double().cpu()

    rm, rvar = bn[2].double().clone(), bn[3].double().clone()
    ref = F.batch_norm(yv.double(), rm, rvar, bn[0].double(), bn[1].double(), True, MOM, EPS)
    if with_res:
        ref = ref + rv_.double()
    if relu:
        ref = ref.clamp_min(0)
    mask = None
    if drop_p > 0:
        mask = torch.from_numpy(dropout_scale(drop_p, DROP_SEED, 3, np.arange((M // rpi) * Cc))).reshape(-1, Cc)
        ref = ref * mask.double().repeat_interleave(rpi, 0)
    # statistics and the rewritten eval fold (bn_train.hip: esc = gamma / sqrt(rv + eps), beta - rm * esc)
    bn_new = bn_d.cpu()
    assert torch.equal(bn_new[:2], bn[:2])
    esc = bn[0].double() / torch.sqrt(rvar + EPS)
    errs = dict(rm=rel(bn_new[2], rm), rv=rel(bn_new[3], rvar), scale=rel(scale, esc),
                shift=rel(shift, bn[1].double() - rm * esc))
    print(f"bn_train M={M} C={Cc} layout={layout}: {errs}, out rel {rel(got, ref):.3e}")
    assert max(errs.values()) < TOL_F32, errs
    d, top = (got - ref).abs(), float(ref.abs().max())
    if layout == ACT_F32:
        assert float(d.max()) / top < TOL_F32
    elif layout == ACT_BF16:  # one bf16 rounding of the float64 value
        assert bool((d <= 2.0 ** -8 * ref.abs() + 1e-6 * top).all()), float((d / ref.abs().clamp_min(1e-3)).max())
    else:  # hi + lo carries 16 bits; the 1e-6 max|ref| floor is the fp32 arithmetic's error where
        # bn(y) cancels to near zero (the same floor as the bf16 bar)
        assert bool((d <= 2.0 ** -15 * ref.abs() + 1e-6 * top).all()), float((d / ref.abs().clamp_min(1e-3)).max())
    if mask is not None:
        assert 0.35 < float((mask == 0).float().mean()) < 0.65
        zero = got.reshape(-1, rpi, Cc).abs().amax(1) == 0
        if relu:  # a kept plane may be all zero behind the ReLU
            assert bool(zero[mask == 0].all()) and torch.equal(zero, ref.reshape(-1, rpi, Cc).abs().amax(1) == 0)
        else:
            assert torch.equal(zero, mask == 0)


# --------------------------------------------------------------------------------------------
# bf16 -> fp32 widen
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 1000003])
def test_widen_bf16(dev, n):
    g = torch.Generator().manual_seed(6000 + n)
    x = (torch.randn(n, generator=g) * 10).to(torch.bfloat16)
    out = torch.full((n + 8,), float("nan"), device=dev)
    op(5, [x.to(dev), out], [n])
    o = out.cpu()
    assert torch.equal(o[:n], x.float()) and bool(torch.isnan(o[n:]).all())
