"""GPU parity of the GroupNorm kernels (tdn_gn_fwd / tdn_gn_bwd) against torch.nn.functional.group_norm (fp32, CPU)
on identical 16-bit-representable inputs.  Tolerances: outputs are 16-bit, so <= 1 ulp of the output type relative to
the fp32 reference (2^-7 bf16 / 2^-10 fp16) + the reduction noise; dgamma / dbeta (fp32) rel-L2 <= 1e-3.

The second half of the file compares GroupNorm and training-mode BatchNorm with the float64 oracle tests/norm_ref.py:
every branch of the launch geometry (GEOM_CASES), inputs whose |mean| / std is in the hundreds (COND_CASES), and the
options of the two entry points; the criteria are stated where that half begins."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from golden_util import _hash_u01, det_tensor, max_rel, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from torch_detection_amd import ops as _ops
    return _ops


CASES = [  # N, C, H, W
    (2, 64, 13, 21),     # 2 channels per group: a lane's 8 channels span 4 groups
    (1, 128, 25, 42),
    (2, 256, 16, 24),
    (2, 512, 7, 9),
    (1, 2048, 4, 5),     # one pixel per block pass
]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", CASES)
def test_gn_fwd_bwd(ops, case, dt):
    N, C, H, W = case
    G = 32
    ulp = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
    rq = lambda t: t.to(dt).float()   # noqa: E731
    z = rq(det_tensor((N, C, H, W), 1, -2, 2, bf16=False) + 0.3).requires_grad_(True)
    gamma = det_tensor((C,), 2, 0.5, 1.5, bf16=False).requires_grad_(True)
    beta = det_tensor((C,), 3, -0.5, 0.5, bf16=False).requires_grad_(True)
    res = rq(det_tensor((N, C, H, W), 4, -1, 1, bf16=False))
    nh = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().to(dt).cuda()   # noqa: E731
    nc = lambda t: t.float().cpu().permute(0, 3, 1, 2).contiguous()            # noqa: E731
    pre = F.group_norm(z, G, gamma, beta, 1e-5)
    ref = F.relu(pre + res)
    y, stats = ops.gn_fwd(nh(z), gamma.detach().cuda(), beta.detach().cuda(), G, 1e-5, nh(res), True)
    assert y.dtype == dt and tuple(stats.shape) == (N, C, 2)
    err = (nc(y) - ref.detach()).abs()
    assert bool((err <= ref.detach().abs() * ulp + 1e-5 * float(ref.abs().max())).all())
    # statistics themselves
    zg = z.detach().view(N, G, -1)
    assert torch.allclose(stats[:, ::C // G, 0].cpu(), zg.mean(-1), rtol=1e-5, atol=1e-6)
    assert torch.allclose(stats[:, ::C // G, 1].cpu(), 1.0 / torch.sqrt(zg.var(-1, unbiased=False) + 1e-5), rtol=1e-5)
    # no addend, no relu
    y0, _ = ops.gn_fwd(nh(z), gamma.detach().cuda(), beta.detach().cuda(), G)
    assert bool(((nc(y0) - pre.detach()).abs() <= pre.detach().abs() * ulp + 1e-5 * float(pre.abs().max())).all())
    # FPN top-down form: + nearest-2x upsampled coarser level
    if H % 2 == 0 and W % 2 == 0:
        coarse = rq(det_tensor((N, C, H // 2, W // 2), 6, -1, 1, bf16=False))
        ref_u = pre.detach() + F.interpolate(coarse, scale_factor=2, mode="nearest")
        yu, _ = ops.gn_fwd(nh(z), gamma.detach().cuda(), beta.detach().cuda(), G, 1e-5, nh(coarse), False, ops.ADD_UP2X)
        assert bool(((nc(yu) - ref_u).abs() <= ref_u.abs() * ulp + 1e-5 * float(ref_u.abs().max())).all())
    # backward: g = cotangent masked by the ReLU (what the consumer's dgrad epilogue hands over)
    cot = rq(det_tensor((N, C, H, W), 5, -1, 1, bf16=False))
    g = rq(cot * (ref.detach() > 0).float())
    pre.backward(g)
    dz, dg, db = ops.gn_bwd(nh(g), nh(z), stats, gamma.detach().cuda(), G)
    assert dz.dtype == dt
    assert rel_l2(dg.cpu(), gamma.grad) <= 1e-3 and rel_l2(db.cpu(), beta.grad) <= 1e-3
    assert max_rel(nc(dz), z.grad) <= 2 * ulp
    # accumulate into existing affine grads
    _, dg2, db2 = ops.gn_bwd(nh(g), nh(z), stats, gamma.detach().cuda(), G, dg.clone(), db.clone(), True)
    assert rel_l2(dg2.cpu(), 2 * gamma.grad) <= 1e-3 and rel_l2(db2.cpu(), 2 * beta.grad) <= 1e-3


def test_gn_bad_shapes(ops):
    z = torch.zeros(1, 4, 4, 96, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(96, device="cuda")
    with pytest.raises(RuntimeError):
        ops.gn_fwd(z, w, w, 32)       # 96 channels: not a power of two
    z = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.gn_fwd(z, w, w, 48)       # groups do not divide channels
    for C, G in ((32, 32), (4096, 32), (2048, 4)):   # below / above the channel range; 512 channels per group
        z = torch.zeros(1, 2, 2, C, dtype=torch.bfloat16, device="cuda")
        w = torch.ones(C, device="cuda")
        with pytest.raises(RuntimeError):
            ops.gn_fwd(z, w, w, G)
        with pytest.raises(RuntimeError):
            ops.gn_bwd(z, z, torch.zeros(1, C, 2, device="cuda"), w, G)
    z = torch.zeros(1, 4, 6, 64, dtype=torch.bfloat16, device="cuda")
    zo = torch.zeros(1, 4, 5, 64, dtype=torch.bfloat16, device="cuda")
    coarse = torch.zeros(1, 2, 2, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.gn_fwd(zo, w, w, 32, 1e-5, coarse, False, ops.ADD_UP2X)     # UP2X with odd W
    with pytest.raises(RuntimeError):
        ops.bn_train_fwd(zo, w, w, None, None, 0.1, 1e-5, coarse, False, ops.ADD_UP2X)
    for bad in (torch.zeros(1, 64, device="cuda"), torch.zeros(1, 32, 2, device="cuda"),
                torch.zeros(2, 64, 2, device="cuda"), torch.zeros(1, 2, 64, device="cuda")):
        with pytest.raises(RuntimeError):
            ops.gn_bwd(z, z, bad, w, 32)                                # stats of the wrong shape
        with pytest.raises(RuntimeError):
            ops.bn_train_bwd(z, z, bad, w)


@pytest.mark.parametrize("case", [(2, 64, 13, 21), (3, 256, 8, 12), (1, 1024, 5, 4)])
def test_bn_train_fwd_bwd(ops, case):
    """Training-mode BatchNorm2d (batch statistics, running-stat update) against F.batch_norm(training=True)."""
    N, C, H, W = case
    dt, ulp = torch.bfloat16, 2.0 ** -7
    rq = lambda t: t.to(dt).float()   # noqa: E731
    z = rq(det_tensor((N, C, H, W), 1, -2, 2, bf16=False) + 0.3).requires_grad_(True)
    gamma = det_tensor((C,), 2, 0.5, 1.5, bf16=False).requires_grad_(True)
    beta = det_tensor((C,), 3, -0.5, 0.5, bf16=False).requires_grad_(True)
    rm0 = det_tensor((C,), 4, -0.2, 0.2, bf16=False)
    rv0 = det_tensor((C,), 5, 0.5, 1.5, bf16=False)
    res = rq(det_tensor((N, C, H, W), 6, -1, 1, bf16=False))
    nh = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().to(dt).cuda()   # noqa: E731
    nc = lambda t: t.float().cpu().permute(0, 3, 1, 2).contiguous()            # noqa: E731
    rm, rv = rm0.clone(), rv0.clone()
    pre = F.batch_norm(z, rm, rv, gamma, beta, True, 0.1, 1e-5)
    ref = F.relu(pre + res)
    rmg, rvg = rm0.clone().cuda(), rv0.clone().cuda()
    y, stats = ops.bn_train_fwd(nh(z), gamma.detach().cuda(), beta.detach().cuda(), rmg, rvg, 0.1, 1e-5, nh(res), True)
    err = (nc(y) - ref.detach()).abs()
    assert bool((err <= ref.detach().abs() * ulp + 1e-5 * float(ref.detach().abs().max())).all())
    assert torch.allclose(rmg.cpu(), rm, rtol=1e-5, atol=1e-6) and torch.allclose(rvg.cpu(), rv, rtol=1e-5, atol=1e-6)
    cot = rq(det_tensor((N, C, H, W), 7, -1, 1, bf16=False))
    g = rq(cot * (ref.detach() > 0).float())
    pre.backward(g)
    dz, dg, db = ops.bn_train_bwd(nh(g), nh(z), stats, gamma.detach().cuda())
    assert rel_l2(dg.cpu(), gamma.grad) <= 1e-3 and rel_l2(db.cpu(), beta.grad) <= 1e-3
    assert max_rel(nc(dz), z.grad) <= 2 * ulp


# ---- float64 oracle (tests/norm_ref.py), launch-geometry branches, ill-conditioned statistics ------------------
# Everything below compares with norm_ref on the same 16-bit-representable inputs.  Criteria:
#   y       |err| <= |ref| * ulp + 1e-5 * max|ref|                       (ulp 2^-7 bf16, 2^-10 fp16; as above)
#   dz      max|err| / max|ref| <= 2 ulp                                 (as above)
#   mean    |err| <= 2^-23 |ref| + 2^-23 std_ref      one fp32 rounding of a value the kernel forms in double
#   rstd    relative error <= 2^-12 in EVERY case: y - beta = gamma * xhat, and 2^-12 is a quarter of the fp16 output
#           ulp, so the statistics never cost a visible fraction of an output ulp
#   dbeta   |err| <= K 2^-24 sum|g|,  dgamma  |err| <= (K 2^-24 + 2^-12) sum|g * xhat_ref|   per channel, K = N*H*W
#           terms: fp32 recursive summation of exactly representable terms, plus the rstd allowance; rel_l2 <= 1e-3 too
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
BF, FP = torch.bfloat16, torch.float16
RSTD_TOL = 2.0 ** -12

GEOM_CASES = [  # N, C, H, W, G, dtype
    (2, 64, 6, 10, 64, BF),       # cpg = 1
    (2, 64, 6, 10, 1, FP),        # cpg = 64, CB = 64
    (1, 128, 9, 7, 4, BF),        # cpg = 32, the CB boundary
    (2, 2048, 3, 2, 8, FP),       # cpg = 256, KL = 1
    (1, 512, 8, 6, 2, BF),        # cpg = 256, two blocks per sample
    (3, 64, 3, 3, 32, FP),        # HW = 9 < 32 pixel lanes
    (2, 64, 1, 1, 32, BF),        # HW = 1
    (1, 64, 37, 41, 32, FP),      # several chunks, ragged last chunk
    (1024, 64, 2, 2, 32, BF),     # chunks forced to 1, gridDim.y = 1024
]
# 2 105 344 lanes > 8192 * 256: the grid-stride loop of both apply kernels iterates, with the UP2X index arithmetic
# inside it.  The smallest even-sided shape over the cap; one dtype, outside the per-dtype product.
BIG_CASE = (1, 64, 514, 512, 32, BF)
BN_GEOM_CASES = [  # N, C, H, W, dtype: the rows above that are not about channels per group
    (3, 64, 3, 3, FP),
    (2, 64, 1, 1, BF),            # N*HW = 2
    (1, 64, 1, 1, FP),            # N*HW = 1: the running variance keeps the biased one (torch refuses this shape)
    (1, 64, 37, 41, BF),
    (1024, 64, 2, 2, FP),
]
BN_BIG_CASE = BIG_CASE[:4] + (BF,)
BN_CASES = [(2, 64, 13, 21), (3, 256, 8, 12), (1, 1024, 5, 4)]
OPT_SHAPE = (3, 256, 8, 12)


def _rq(a, dt):
    """float64 array of the values `a` takes when stored as dt"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt).float().numpy().astype(np.float64)


def _dev(a, dt):
    """NCHW array of dt-representable values -> NHWC device tensor"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


def _host(t):
    return t.float().cpu().permute(0, 3, 1, 2).contiguous().numpy().astype(np.float64)


def _vec(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _det(shape, seed, lo, hi):
    return det_tensor(shape, seed, lo, hi, bf16=False).numpy().astype(np.float64)


def _varied(shape, seed, dt):
    """uniform(-2, 2) scaled by 2^(n % 3) and shifted by 0.3 + n in sample n: no two samples share statistics, so a
    per-sample indexing slip cannot hide"""
    n = np.arange(shape[0], dtype=np.float64).reshape(-1, 1, 1, 1)
    return _rq(_det(shape, seed, -2, 2) * 2.0 ** (n % 3) + 0.3 + n, dt)


def _affine(C):
    return _det((C,), 2, 0.5, 1.5), _det((C,), 3, -0.5, 0.5)     # float32 values: what the kernel is handed


def _check_y(y, ref, ulp, tag):
    err = np.abs(y - ref)
    lim = np.abs(ref) * ulp + 1e-5 * np.abs(ref).max()
    print("%s: y worst err/limit %.3g" % (tag, float((err / np.maximum(lim, 1e-300)).max())))
    assert bool((err <= lim).all()), tag


def _check_stats(stats, mean, rstd, std, tag, rstd_tol=RSTD_TOL):
    """stats (N, C, 2) from the device against per-(sample, channel) float64 mean / rstd / std"""
    s = stats.cpu().numpy().astype(np.float64)
    assert s.shape == mean.shape + (2,), tag
    em = np.abs(s[..., 0] - mean)
    lm = 2.0 ** -23 * np.abs(mean) + 2.0 ** -23 * std
    er = np.abs(s[..., 1] - rstd) / rstd
    print("%s: mean worst err/limit %.3g, rstd worst rel err %.3g" %
          (tag, float((em / np.maximum(lm, 1e-300)).max()) if em.max() > 0 else 0.0, float(er.max())))
    assert bool((em <= lm).all()), tag + " mean"
    assert float(er.max()) <= rstd_tol, tag + " rstd"


def _check_bwd(dz, dg, db, ref, g, xhat, ulp, tag):
    rdz, rdg, rdb = ref
    K = g.shape[0] * g.shape[2] * g.shape[3]
    den = np.abs(rdz).max()
    mr = float(np.abs(dz - rdz).max() / (den if den > 0 else 1.0))
    edg, edb = np.abs(dg - rdg), np.abs(db - rdb)
    ldb = K * 2.0 ** -24 * np.abs(g).sum((0, 2, 3))
    ldg = (K * 2.0 ** -24 + 2.0 ** -12) * np.abs(g * xhat).sum((0, 2, 3))
    l2g, l2b = rel_l2(torch.from_numpy(dg), torch.from_numpy(rdg)), rel_l2(torch.from_numpy(db), torch.from_numpy(rdb))
    print("%s: dz max_rel %.3g (limit %.3g), dgamma worst err/limit %.3g rel_l2 %.3g, dbeta worst err/limit %.3g "
          "rel_l2 %.3g" % (tag, mr, 2 * ulp, float((edg / np.maximum(ldg, 1e-300)).max()) if edg.max() > 0 else 0.0,
                           l2g, float((edb / np.maximum(ldb, 1e-300)).max()) if edb.max() > 0 else 0.0, l2b))
    assert mr <= 2 * ulp, tag + " dz"
    assert bool((edb <= ldb).all()), tag + " dbeta"
    assert bool((edg <= ldg).all()), tag + " dgamma"
    assert l2g <= 1e-3 and l2b <= 1e-3, tag + " rel_l2"


def _f64(t):
    return t.cpu().numpy().astype(np.float64)


def run_gn(ops, z, G, dt, eps=1e-5, addend=None, up2x=False, relu=0, tag="gn", exact_y=None):
    """One GroupNorm forward + backward on the device against norm_ref; z (and addend) hold dt-representable values."""
    N, C, H, W = z.shape
    ulp, cpg = ULP[dt], C // G
    gamma, beta = _affine(C)
    ref, mean, rstd = R.gn_fwd(z, gamma, beta, G, eps, addend, up2x, relu)
    std = np.sqrt(np.maximum(rstd ** -2 - eps, 0.0))
    mode = ops.ADD_UP2X if up2x else ops.ADD_SAME
    y, stats = ops.gn_fwd(_dev(z, dt), _vec(gamma), _vec(beta), G, eps, None if addend is None else _dev(addend, dt),
                          relu, mode)
    assert y.dtype == dt and tuple(stats.shape) == (N, C, 2)
    _check_stats(stats, mean.repeat(cpg, 1), rstd.repeat(cpg, 1), std.repeat(cpg, 1), tag)
    if exact_y is not None:
        exact_y(_host(y))
    _check_y(_host(y), ref, ulp, tag)
    g = _rq(_det(z.shape, 5, -1, 1) * (ref > 0 if relu else 1.0), dt)
    dz, dg, db = ops.gn_bwd(_dev(g, dt), _dev(z, dt), stats, _vec(gamma), G)
    assert dz.dtype == dt
    xhat = ((z.reshape(N, G, -1) - mean[..., None]) * rstd[..., None]).reshape(z.shape)
    _check_bwd(_host(dz), _f64(dg), _f64(db), R.gn_bwd(g, z, gamma, G, eps), g, xhat, ulp, tag)


def run_bn(ops, z, dt, eps=1e-5, addend=None, up2x=False, relu=0, momentum=0.1, running=True, tag="bn",
           exact_y=None):
    """One training-mode BatchNorm forward + backward on the device against norm_ref."""
    N, C, H, W = z.shape
    ulp = ULP[dt]
    gamma, beta = _affine(C)
    rm0, rv0 = (_det((C,), 4, -0.2, 0.2), _det((C,), 5, 0.5, 1.5)) if running else (None, None)
    ref, mean, rstd, rm, rv = R.bn_train_fwd(z, gamma, beta, eps, addend, up2x, relu, rm0, rv0, momentum)
    std = np.sqrt(np.maximum(rstd ** -2 - eps, 0.0))
    rmg, rvg = (_vec(rm0), _vec(rv0)) if running else (None, None)
    mode = ops.ADD_UP2X if up2x else ops.ADD_SAME
    y, stats = ops.bn_train_fwd(_dev(z, dt), _vec(gamma), _vec(beta), rmg, rvg, momentum, eps,
                                None if addend is None else _dev(addend, dt), relu, mode)
    assert y.dtype == dt and tuple(stats.shape) == (N, C, 2)
    rep = lambda v: np.broadcast_to(v, (N, C))   # noqa: E731
    _check_stats(stats, rep(mean), rep(rstd), rep(std), tag)
    if running:
        print("%s: running mean worst abs err %.3g, running var worst rel err %.3g" %
              (tag, float(np.abs(_f64(rmg) - rm).max()), float((np.abs(_f64(rvg) - rv) / np.abs(rv)).max())))
        assert np.allclose(_f64(rmg), rm, rtol=1e-5, atol=1e-6) and np.allclose(_f64(rvg), rv, rtol=1e-5, atol=1e-6)
    if exact_y is not None:
        exact_y(_host(y))
    _check_y(_host(y), ref, ulp, tag)
    g = _rq(_det(z.shape, 7, -1, 1) * (ref > 0 if relu else 1.0), dt)
    dz, dg, db = ops.bn_train_bwd(_dev(g, dt), _dev(z, dt), stats, _vec(gamma))
    assert dz.dtype == dt
    xhat = (z - mean[None, :, None, None]) * rstd[None, :, None, None]
    _check_bwd(_host(dz), _f64(dg), _f64(db), R.bn_train_bwd(g, z, gamma, eps), g, xhat, ulp, tag)


def _gid(case):
    return "-".join("bf16" if v is BF else "fp16" if v is FP else str(v) for v in case)


@pytest.mark.parametrize("case", GEOM_CASES, ids=_gid)
def test_gn_geometry(ops, case):
    """Every branch of the launch geometry (channels per group 1 .. 256, HW below the pixel lanes, one chunk, many
    samples), with a same-size addend and ReLU, samples of different statistics."""
    N, C, H, W, G, dt = case
    run_gn(ops, _varied((N, C, H, W), 1, dt), G, dt, addend=_rq(_det((N, C, H, W), 4, -1, 1), dt), relu=1,
           tag="gn " + _gid(case))


def test_gn_grid_stride(ops):
    """More 8-channel lanes than the capped grid has threads: both apply kernels loop, with the UP2X addend."""
    N, C, H, W, G, dt = BIG_CASE
    run_gn(ops, _varied((N, C, H, W), 1, dt), G, dt, addend=_rq(_det((N, C, H // 2, W // 2), 6, -1, 1), dt), up2x=True,
           relu=1, tag="gn " + _gid(BIG_CASE))


@pytest.mark.parametrize("case", BN_GEOM_CASES, ids=_gid)
def test_bn_train_geometry(ops, case):
    N, C, H, W, dt = case
    run_bn(ops, _varied((N, C, H, W), 1, dt), dt, addend=_rq(_det((N, C, H, W), 6, -1, 1), dt), relu=1,
           tag="bn " + _gid(case))


def test_bn_train_grid_stride(ops):
    N, C, H, W, dt = BN_BIG_CASE
    run_bn(ops, _varied((N, C, H, W), 1, dt), dt, addend=_rq(_det((N, C, H // 2, W // 2), 6, -1, 1), dt), up2x=True,
           relu=1, tag="bn " + _gid(BN_BIG_CASE))


# ---- ill-conditioned statistics: values m + k * ulp16(m), integer k from the hash, |mean| / std in the hundreds ----
COND_SHAPES = [(1, 64, 32, 32), (2, 256, 16, 24)]
COND_ROWS = [  # name, dtype, m, largest |k|, least |mean| / std the row must have (None: not claimed)
    ("fp16-m8-k6", FP, 8.0, 6, None),
    ("fp16-m8-k2", FP, 8.0, 2, 250.0),
    ("fp16-m64-k3", FP, 64.0, 3, 250.0),
    ("fp16-m-8-k2", FP, -8.0, 2, 250.0),
    ("bf16-m8-k2", BF, 8.0, 2, None),
]
COND_CASES = [(name, dt, m, kmax, need, shape) for name, dt, m, kmax, need in COND_ROWS for shape in COND_SHAPES]


def ulp16(m, dt):
    return 2.0 ** (np.floor(np.log2(abs(m))) - (7 if dt is BF else 10))


def cond_input(shape, dt, m, kmax, seed=11):
    n = int(np.prod(shape))
    k = np.floor(_hash_u01(n, seed).astype(np.float64) * (2 * kmax + 1)) - kmax
    z = (m + k * ulp16(m, dt)).reshape(shape)
    assert np.array_equal(z, _rq(z, dt)), "not representable"
    return z


def _cond_ratio_gn(z, G):
    mu, _, var = R.gn_stats(z, G, 0.0)
    return float((np.abs(mu) / np.sqrt(var)).min())


def _cond_ratio_bn(z):
    mu, _, var = R.bn_stats(z, 0.0)
    return float((np.abs(mu) / np.sqrt(var)).min())


for _name, _dt, _m, _kmax, _need, _shape in COND_CASES:     # at collection, on the CPU: the rows stress what they claim
    if _need is not None:
        _z = cond_input(_shape, _dt, _m, _kmax)
        assert _cond_ratio_gn(_z, 32) >= _need and _cond_ratio_bn(_z) >= _need, (_name, _shape)


def _cid(case):
    return "%s-%s" % (case[0], "x".join(str(v) for v in case[5]))


@pytest.mark.parametrize("case", COND_CASES, ids=_cid)
def test_gn_ill_conditioned(ops, case):
    name, dt, m, kmax, _, shape = case
    run_gn(ops, cond_input(shape, dt, m, kmax), 32, dt, tag="gn cond " + _cid(case))


@pytest.mark.parametrize("case", COND_CASES, ids=_cid)
def test_bn_train_ill_conditioned(ops, case):
    name, dt, m, kmax, _, shape = case
    run_bn(ops, cond_input(shape, dt, m, kmax), dt, tag="bn cond " + _cid(case))


def _const_input(shape, cpg):
    """channel blocks of cpg channels, alternately constant (8) and 8 + k ulp, k in [-2, 2]"""
    z = cond_input(shape, FP, 8.0, 2)
    z[:, (np.arange(shape[1]) // cpg) % 2 == 0] = 8.0
    return z


@pytest.mark.parametrize("shape", COND_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["gn", "bn"])
def test_constant_group(ops, kind, shape):
    """A constant group (channel, for BN): rstd = 1/sqrt(eps), and the output is the rounded beta + addend exactly."""
    N, C, H, W = shape
    cpg = C // 32
    z = _const_input(shape, cpg)
    const = (np.arange(C) // cpg) % 2 == 0
    addend = _rq(_det(shape, 4, -1, 1), FP)
    _, beta = _affine(C)
    want = (torch.from_numpy(beta.astype(np.float32))[None, :, None, None] +
            torch.from_numpy(addend.astype(np.float32))).half().float().numpy().astype(np.float64)

    def exact(y):
        assert np.array_equal(y[:, const], want[:, const]), "constant group: y != round(beta + addend)"

    if kind == "gn":
        _, _, rstd = R.gn_fwd(z, beta, beta, 32, 1e-5)
        assert np.allclose(rstd[:, ::2], 1e-5 ** -0.5, rtol=1e-12)
        run_gn(ops, z, 32, FP, addend=addend, tag="gn const", exact_y=exact)
    else:
        run_bn(ops, z, FP, addend=addend, tag="bn const", exact_y=exact)


@pytest.mark.parametrize("shape", COND_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["gn", "bn"])
def test_opposite_pivots(ops, kind, shape):
    """Two channels per group, one at +8 +- 2 ulp and one at -8 +- 2 ulp: group mean ~ 0, variance ~ 64.  Well
    conditioned as a group, but each channel is far from the group mean: the cross terms between channels count."""
    N, C, H, W = shape
    z = cond_input(shape, FP, 8.0, 2)
    z[:, 1::2] *= -1.0
    if kind == "gn":
        mu, _, var = R.gn_stats(z, C // 2, 0.0)
        assert float(np.abs(mu).max()) < 0.01 and float(np.abs(var - 64).max()) < 0.1
        run_gn(ops, z, C // 2, FP, tag="gn opposite")
    else:
        run_bn(ops, z, FP, tag="bn opposite")


# ---- options of the two entry points, one small shape each ------------------------------------------------------
@pytest.mark.parametrize("case", BN_CASES)
def test_bn_train_fp16(ops, case):
    run_bn(ops, _varied(case, 1, FP), FP, addend=_rq(_det(case, 6, -1, 1), FP), relu=1, tag="bn fp16 %s" % (case,))


@pytest.mark.parametrize("momentum", [0.25, 1.0])
def test_bn_train_momentum(ops, momentum):
    run_bn(ops, _varied(OPT_SHAPE, 1, BF), BF, momentum=momentum, tag="bn momentum %g" % momentum)


def test_bn_train_no_running_stats(ops):
    run_bn(ops, _varied(OPT_SHAPE, 1, BF), BF, running=False, addend=_rq(_det(OPT_SHAPE, 6, -1, 1), BF), relu=1,
           tag="bn no running stats")


@pytest.mark.parametrize("kind", ["gn", "bn"])
def test_eps(ops, kind):
    z = _varied(OPT_SHAPE, 1, FP)
    if kind == "gn":
        run_gn(ops, z, 32, FP, eps=1e-3, tag="gn eps 1e-3")
    else:
        run_bn(ops, z, FP, eps=1e-3, tag="bn eps 1e-3")


@pytest.mark.parametrize("kind", ["gn", "bn"])
@pytest.mark.parametrize("dt", [BF, FP], ids=["bf16", "fp16"])
def test_relu6(ops, kind, dt):
    """ReLU6.  Values stored under 6 stay under 6 (relu6_top, common.h), so compare below the knee and at the clamp,
    as test_gpu_halo.py does.  The affine is scaled so that a fair share of the outputs sits at the clamp."""
    N, C, H, W = OPT_SHAPE
    z = _varied(OPT_SHAPE, 1, dt)
    gamma, beta = _det((C,), 2, 3.0, 9.0), _det((C,), 3, 1.5, 2.5)
    if kind == "gn":
        ref, _, _ = R.gn_fwd(z, gamma, beta, 32, 1e-5, relu=2)
        y, _ = ops.gn_fwd(_dev(z, dt), _vec(gamma), _vec(beta), 32, 1e-5, None, 2)
    else:
        ref, _, _, _, _ = R.bn_train_fwd(z, gamma, beta, 1e-5, relu=2)
        y, _ = ops.bn_train_fwd(_dev(z, dt), _vec(gamma), _vec(beta), None, None, 0.1, 1e-5, None, 2)
    share = float((ref >= 6).mean())
    print("%s relu6 %s: share at the clamp %.3f, at zero %.3f" % (kind, dt, share, float((ref <= 0).mean())))
    assert 0.05 <= share <= 0.95
    y = _host(y)
    low = ref < 5.9
    err = np.abs(y - ref)
    assert bool((err[low] <= np.abs(ref[low]) * ULP[dt] + 1e-5 * 6).all())
    assert bool((y[ref >= 6] == 6).all()) and float(y.max()) <= 6 and float(y.min()) >= 0


def test_bn_train_up2x(ops):
    N, C, H, W = OPT_SHAPE
    run_bn(ops, _varied(OPT_SHAPE, 1, BF), BF, addend=_rq(_det((N, C, H // 2, W // 2), 6, -1, 1), BF), up2x=True,
           tag="bn up2x")


@pytest.mark.parametrize("kind", ["gn", "bn"])
def test_accumulate_and_overwrite(ops, kind):
    """accumulate=True adds the gradients onto whatever the buffers hold (expected: base + float64 gradient, within
    the gradient's own bound and one fp32 rounding of the sum); accumulate=False into the same buffers overwrites,
    and repeats the first result bit for bit (fixed summation order)."""
    N, C, H, W = OPT_SHAPE
    dt = BF
    z = _varied(OPT_SHAPE, 1, dt)
    gamma, beta = _affine(C)
    g = _rq(_det(OPT_SHAPE, 5, -1, 1), dt)
    if kind == "gn":
        _, stats = ops.gn_fwd(_dev(z, dt), _vec(gamma), _vec(beta), 32)
        bwd = lambda *a: ops.gn_bwd(_dev(g, dt), _dev(z, dt), stats, _vec(gamma), 32, *a)    # noqa: E731
        _, rdg, rdb = R.gn_bwd(g, z, gamma, 32, 1e-5)
        xhat = R.gn_xhat(z, 32, 1e-5)
    else:
        _, stats = ops.bn_train_fwd(_dev(z, dt), _vec(gamma), _vec(beta))
        bwd = lambda *a: ops.bn_train_bwd(_dev(g, dt), _dev(z, dt), stats, _vec(gamma), *a)  # noqa: E731
        _, rdg, rdb = R.bn_train_bwd(g, z, gamma, 1e-5)
        mu, rstd, _ = R.bn_stats(z, 1e-5)
        xhat = (z - mu[None, :, None, None]) * rstd[None, :, None, None]
    K = N * H * W
    ldb = K * 2.0 ** -24 * np.abs(g).sum((0, 2, 3))
    ldg = (K * 2.0 ** -24 + 2.0 ** -12) * np.abs(g * xhat).sum((0, 2, 3))
    dz0, dg0, db0 = bwd()
    base_g, base_b = _det((C,), 8, -30, 30).astype(np.float32), _det((C,), 9, -30, 30).astype(np.float32)
    bg, bb = _vec(base_g), _vec(base_b)
    _, dg1, db1 = bwd(bg, bb, True)
    assert dg1.data_ptr() == bg.data_ptr() and db1.data_ptr() == bb.data_ptr()
    wg, wb = base_g.astype(np.float64) + rdg, base_b.astype(np.float64) + rdb
    assert bool((np.abs(_f64(bg) - wg) <= ldg + 2.0 ** -23 * np.abs(wg)).all())
    assert bool((np.abs(_f64(bb) - wb) <= ldb + 2.0 ** -23 * np.abs(wb)).all())
    dz2, _, _ = bwd(bg, bb, False)
    assert torch.equal(bg, dg0) and torch.equal(bb, db0) and torch.equal(dz2.view(torch.int16), dz0.view(torch.int16))
