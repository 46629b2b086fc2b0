"""Every bf16x6 kernel body (fp32 operands split into three bf16 parts, the six products
a_i b_j, i + j <= 2, on v_mfma_f32_16x16x32_bf16; three or one of them for bf16 operands) on
operands that reveal a missing or mis-paired product: tests/_x6_ref.py plants operands whose
three parts are all large and one-signed per output element, and tests/test_cpu_x6_inputs.py
proves on the same table of cases that the full product set lands within 0.1 bound of the fp64
product while every single-product mutant is off by >= 3 bound at every element. Here the kernel
output is compared per element with the fp64 product of the same operands against
bound = 2e-6 (|a| @ |b| + |bias|), the tolerance of tests/test_gpu_gemm.py, for the plain family
and for its signed form. Each test prints its largest error / bound (pytest -s).

A result stored in bf16 (regnn_type_project and regnn_head_bwd_z's gh with bf16 rows) cannot be
held to `bound` itself: it must be a bf16 rounding of some fp32 value within bound of the fp64
product (_x6_ref.bf16_window). A lost first-order product moves the value by 0.4 to 1 bf16 ulp
and takes more than a quarter of the elements out of that window (asserted on the CPU); a
second-order one only the few elements next to a rounding tie. So the second-order product w2 x0
of type_project_kernel<bf16> and the second-order gh products of the bf16 ZP kernel are NOT
reliably revealed (the CPU test prints how many elements each would move); the source lines of
those products are shared with the fp32 instances of the same templates, which are held to
bound."""
import numpy as np
import pytest
import torch

import _x6_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
SGN = pytest.mark.parametrize("sgn", [0, 1], ids=["plain", "signed"])
DTYPE = pytest.mark.parametrize("dtype", ["fp32", "bf16"])
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]


def _t(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(dtype)


def _np(t):
    torch.cuda.synchronize()
    return t.detach().double().cpu().numpy()


def _check(tag, got, ref, bnd):
    """|got - ref| <= bnd at every element (bnd > 0 everywhere)."""
    got = _np(got)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert (bnd > 0).all(), tag
    ratio = np.abs(got - ref) / bnd
    worst = float(ratio.max()) if np.isfinite(ratio).all() else float("inf")
    print(f"X6GPU {tag} max err/bound {worst:.4f}")
    assert worst <= 1.0, (tag, worst, np.unravel_index(int(np.nanargmax(ratio)), ratio.shape))


def _check_pair(tag, got, pr):
    _check(f"{tag}/{pr.name} [{pr.body}]", got, pr.exact(), pr.bound())


def _check_window(tag, got, pr):
    """a bf16-stored result: a rounding of some fp32 value within bound of the fp64 product."""
    assert got.dtype == torch.bfloat16
    g = _np(got).astype(np.float32)
    lo, hi = X.bf16_window(pr.exact(), pr.bound())
    bad = ~((g >= lo) & (g <= hi))
    print(f"X6GPU {tag}/{pr.name} [{pr.body}] bf16 results outside the bound's window: "
          f"{int(bad.sum())} of {bad.size}")
    assert not bad.any(), (tag, int(bad.sum()))


def _tag(key, sgn, extra=""):
    return f"{X.case_id(key)}/{'signed' if sgn else 'plain'}{extra}"


def _stored(x, trans):
    return _t(x.T if trans else x)


# ---------------------------------------------------------------------------------------------
# regnn_gemm_x6 through ops.gemm_x6
@SGN
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("shape", X.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_x6_products(shape, ta, tb, sgn, monkeypatch):
    """(16,16,32): one MFMA tile, the NI = NJ = 1 edge body; (130,132,64): second row / column
    tiles of 2 / 4 valid lines; (150,200,96): 2 or 3 of 4 wave tiles valid, run as 4;
    (65,35,33): no contiguous dimension a multiple of 4, the per-element load forms;
    (130,132,256): split-K in 2 and in 3."""
    from regnn_hip import ops
    key = ("gemm",) + shape
    case = X.build(key, sgn)
    a, b = _stored(case.a, ta), _stored(case.b, tb)
    if shape[2] == 256:
        for s in (2, 3):
            monkeypatch.setattr(ops, "_gemm_splits", lambda *_, s=s: s)
            c = ops.gemm_x6(a, b, trans_a=ta, trans_b=tb)
            _check_pair(_tag(key, sgn, f"/ta{int(ta)}tb{int(tb)}/splits{s}"), c, case.pairs[0])
    else:
        assert ops._gemm_splits(*shape) == 1
        c = ops.gemm_x6(a, b, trans_a=ta, trans_b=tb)
        _check_pair(_tag(key, sgn, f"/ta{int(ta)}tb{int(tb)}"), c, case.pairs[0])


@SGN
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_x6_products_live_rows(ta, tb, sgn, monkeypatch):
    """m_live = 70 of 200 rows (rows >= 70 of op(a) zero): the 64-row tiling, then
    REGNN_GEMM_BM64=off (128-row tiles); the dead rows of C are zeros."""
    from regnn_hip import ops
    key = ("gemm_live",) + X.GEMM_LIVE
    live = X.GEMM_LIVE[3]
    case = X.build(key, sgn)
    a, b = _stored(case.a, ta), _stored(case.b, tb)
    monkeypatch.setattr(ops, "_gemm_splits", lambda *_: 1)
    cnt = torch.tensor([live], dtype=torch.int32, device=DEV)
    for mode in ("on", "off"):
        monkeypatch.setenv("REGNN_GEMM_BM64", mode)
        c = ops.gemm_x6(a, b, trans_a=ta, trans_b=tb, m_live=cnt)
        _check_pair(_tag(key, sgn, f"/ta{int(ta)}tb{int(tb)}/bm64{mode}"), c[:live], case.pairs[0])
        assert not c[live:].any()


def _gemm_call(M, N, K, a, lda, b, ldb, c, ldc, beta=0.0, splits=1, k_live=None):
    from regnn_hip import _lib as L
    work = torch.empty(splits * M * N, dtype=torch.float32, device=DEV) if splits > 1 else None
    L.call("regnn_gemm_x6", 0, 0, M, N, K, L.ptr(a), lda, L.ptr(b), ldb, L.ptr(c), ldc,
           float(beta), L.ptr(work), splits, None, L.ptr(k_live), L.stream())


@SGN
def test_gemm_x6_abi_strides_offset_beta(sgn):
    """regnn_gemm_x6 by the ABI, A [M, K] (k contiguous) and B [K, N] (n contiguous): leading
    dimensions larger than the extents (views into NaN-filled buffers, C's padding still NaN
    afterwards); operand bases offset by one float (the per-element instance through the address
    test); beta = 0.5 with 1 and 2 splits (reference + 0.5 c0, bound + 2e-6 |0.5 c0|)."""
    key = ("gemm_abi",) + X.GEMM_ABI
    M, N, K = X.GEMM_ABI
    case = X.build(key, sgn)
    pr = case.pairs[0]
    nan = float("nan")
    ab = torch.full((M, K + 4), nan, device=DEV)
    bb = torch.full((K, N + 4), nan, device=DEV)
    cb = torch.full((M, N + 3), nan, device=DEV)
    ab[:, :K], bb[:, :N] = _t(case.a), _t(case.b)
    _gemm_call(M, N, K, ab, K + 4, bb, N + 4, cb, N + 3)
    _check_pair(_tag(key, sgn, "/ld"), cb[:, :N], pr)
    assert torch.isnan(cb[:, N:]).all()
    af = torch.full((M * K + 1,), nan, device=DEV)
    bf = torch.full((K * N + 1,), nan, device=DEV)
    af[1:], bf[1:] = _t(case.a).reshape(-1), _t(case.b).reshape(-1)
    a1, b1 = af[1:].view(M, K), bf[1:].view(K, N)
    assert a1.data_ptr() % 16 == 4 and b1.data_ptr() % 16 == 4
    c = torch.full((M, N), nan, device=DEV)
    _gemm_call(M, N, K, a1, K, b1, N, c, N)
    _check_pair(_tag(key, sgn, "/offset"), c, pr)
    a, b = _t(case.a), _t(case.b)
    ref = pr.exact() + 0.5 * case.c0.astype(np.float64)
    bnd = pr.bound() + 2e-6 * np.abs(0.5 * case.c0.astype(np.float64))
    for splits in (1, 2):
        c = _t(case.c0)
        _gemm_call(M, N, K, a, K, b, N, c, N, beta=0.5, splits=splits)
        _check(_tag(key, sgn, f"/beta0.5/splits{splits} [{pr.body}]"), c, ref, bnd)


@SGN
def test_gemm_x6_abi_k_live(sgn):
    """k_live = 40 of K = 96 (both operands zero past it): the k-steps past it are skipped."""
    key = ("gemm_klive",) + X.GEMM_KLIVE
    M, N, K, kl = X.GEMM_KLIVE
    case = X.build(key, sgn)
    c = torch.full((M, N), float("nan"), device=DEV)
    cnt = torch.tensor([kl], dtype=torch.int32, device=DEV)
    _gemm_call(M, N, K, _t(case.a), K, _t(case.b), N, c, N, k_live=cnt)
    _check_pair(_tag(key, sgn), c, case.pairs[0])


# ---------------------------------------------------------------------------------------------
# output head forward: logits of regnn_head_fwd, regnn_head_fwd_lse (fp32 and bf16 rows)
@SGN
@DTYPE
@pytest.mark.parametrize("C", X.HEAD_C)
@pytest.mark.parametrize("rows", X.HEAD_ROWS)
def test_head_fwd_logits_products(rows, C, dtype, sgn):
    """class-tile counts 1, 3, 22, 23; rows of 1, 2 and 19 node tiles; bias from the family; the
    rows padded to 16 classes (as ops.head_ce lays them out) and unpadded. bf16 rows: the
    three-product body. The loss and lse stay with the existing tests (no loss rows here)."""
    from regnn_hip import _lib as L
    key = ("head_fwd", rows, C)
    case = X.build(key, sgn)
    fp32, bf16 = case.pairs
    h, hb = _t(case.h), _t(case.hb, torch.bfloat16)
    w, bias = _t(case.w), _t(case.bias)
    for ld in sorted({C, 16 * ((C + 15) // 16)}):
        def buf():
            return torch.full((rows, ld), float("nan"), device=DEV)
        z = buf()
        if dtype == "fp32":
            L.call("regnn_head_fwd", L.ptr(h), rows, 64, L.ptr(w), L.ptr(bias), C, ld, None, 0,
                   1.0, L.ptr(z), None, None, L.stream())
            _check_pair(_tag(key, sgn, f"/ld{ld}/head_fwd"), z[:, :C], fp32)
            z = buf()
            L.call("regnn_head_fwd_lse", L.ptr(h), rows, 64, L.ptr(w), L.ptr(bias), C, ld, None,
                   0, L.ptr(z), None, 0, L.stream())
            _check_pair(_tag(key, sgn, f"/ld{ld}/head_fwd_lse"), z[:, :C], fp32)
            continue
        L.call("regnn_head_fwd_lse", L.ptr(hb), rows, 64, L.ptr(w), L.ptr(bias), C, ld, None, 0,
               L.ptr(z), None, 1, L.stream())
        _check_pair(_tag(key, sgn, f"/ld{ld}/head_fwd_lse"), z[:, :C], bf16)


# ---------------------------------------------------------------------------------------------
# output head backward
def _padded(x, C):
    """[n, C] rows in a zero-padded buffer of ld = 16 ceil(C / 16)."""
    ld = 16 * ((C + 15) // 16)
    buf = torch.zeros(x.shape[0], ld, device=DEV)
    buf[:, :C] = _t(x)
    return buf, ld


def _slab_parts(slab, C):
    from regnn_hip import ops
    Cp = 16 * ((C + 15) // 16)
    tot = ops._reduce(slab, Cp * 64 + Cp)
    return tot[:Cp * 64].view(Cp, 64)[:C], tot[Cp * 64:Cp * 64 + C]


def _check_colsum(tag, got, p):
    p64 = p.astype(np.float64)
    _check(tag + "/gb", got, p64.sum(0), 2e-6 * np.abs(p64).sum(0))


@SGN
@pytest.mark.parametrize("C", X.BWD_C)
@pytest.mark.parametrize("n", X.BWD_N)
def test_head_bwd_planted_p_products(n, C, sgn):
    """regnn_head_bwd and regnn_head_gh_next on a p from the family, so both operands of both
    products are planted: gh = p W per element (rows past n zero), and the reduced slab
    gW = p^T h, gb = colsum p."""
    from regnn_hip import _lib as L
    key = ("head_bwd", n, C)
    case = X.build(key, sgn)
    gh_pair, gw_pair = case.pairs
    p, ld = _padded(case.p, C)
    w, h = _t(case.w), _t(case.h)
    n_out = n + 3
    one = torch.ones(1, device=DEV)
    gh = torch.full((n_out, 64), float("nan"), device=DEV)
    L.call("regnn_head_bwd", L.ptr(p), n, C, ld, 64, L.ptr(w), None, L.ptr(one), L.ptr(gh),
           n_out, None, 0, L.stream())
    _check_pair(_tag(key, sgn, "/head_bwd"), gh[:n], gh_pair)
    assert not gh[n:].any()
    rows = 2048
    Cp = 16 * ((C + 15) // 16)
    slab = torch.zeros(rows, Cp * 64 + Cp, device=DEV)
    L.call("regnn_head_bwd", L.ptr(p), n, C, ld, 64, None, L.ptr(h), None, None, 0, L.ptr(slab),
           rows, L.stream())
    gW, gb = _slab_parts(slab, C)
    _check_pair(_tag(key, sgn, "/head_bwd"), gW, gw_pair)
    _check_colsum(_tag(key, sgn, "/head_bwd"), gb, case.p)
    gh = torch.full((n_out, 64), float("nan"), device=DEV)
    hx = torch.zeros(n_out, 64, device=DEV)
    hx[:n] = h
    post = torch.full((n_out,), 2.0, device=DEV)
    nx_out, nx_dot = torch.empty_like(hx), torch.empty(n_out, device=DEV)
    L.call("regnn_head_gh_next", L.ptr(p), n, C, ld, 64, L.ptr(w), L.ptr(one), L.ptr(gh), n_out,
           L.ptr(post), L.ptr(hx), L.ptr(nx_out), L.ptr(nx_dot), L.stream())
    _check_pair(_tag(key, sgn, "/head_gh_next"), gh[:n], gh_pair)
    assert not gh[n:].any()


@SGN
@DTYPE
@pytest.mark.parametrize("C", X.BWD_C)
@pytest.mark.parametrize("n", X.BWD_N)
def test_head_bwd_z_products(n, C, dtype, sgn):
    """regnn_head_bwd_z forms p = scale (exp(z - lse) - [label]) inside the kernels, so only W
    (for gh = p W) and h (for the slab gW = p^T h) are planted and p is generic; the reference
    is the fp64 product of the fp32 p that formula gives. Revealed (test_cpu_x6_inputs.py): the
    products of p's first part with every part of W / h, and the re-pairings replacing them.
    Not revealed: p1 w0 / p1 h0, p1 w1 / p1 h1, p2 w0 / p2 h0 and the re-pairings of those (a
    generic remainder has random sign and size): they are covered through the stored-p entry
    (test_head_bwd_planted_p_products), whose kernels are the same templates without ZP. With
    bf16 rows the slab's h has one part (three products, p0 h0 revealed) and gh is stored in
    bf16: only its first-order products p0 w0, p0 w1 are revealed (see the module docstring)."""
    from regnn_hip import _lib as L
    key = ("head_bwd_z", n, C)
    case = X.build(key, sgn)
    gh_pair, gw_pair, gw_bf16 = case.pairs
    z, ld = _padded(case.z, C)
    lse = _t(case.lse)
    lab = torch.from_numpy(case.labels.astype(np.int64)).to(DEV)
    w = _t(case.w)
    bf = dtype == "bf16"
    tdt = torch.bfloat16 if bf else torch.float32
    h = _t(case.hb if bf else case.h, tdt)
    code = 1 if bf else 0
    n_out = n + 3
    one = torch.ones(1, device=DEV)
    gh = torch.full((n_out, 64), float("nan"), device=DEV, dtype=tdt)
    L.call("regnn_head_bwd_z", L.ptr(z), n, C, ld, 64, L.ptr(w), L.ptr(h), L.ptr(one), L.ptr(gh),
           n_out, None, 0, L.ptr(lse), L.ptr(lab), X.ZP_SCALE, None, None, None, None, code,
           L.stream())
    tag = _tag(key, sgn, f"/{dtype}")
    if bf:
        _check_window(tag, gh[:n], gh_pair)
    else:
        _check_pair(tag, gh[:n], gh_pair)
    assert not gh[n:].any()
    rows = 2048
    Cp = 16 * ((C + 15) // 16)
    slab = torch.zeros(rows, Cp * 64 + Cp, device=DEV)
    L.call("regnn_head_bwd_z", L.ptr(z), n, C, ld, 64, None, L.ptr(h), None, None, 0,
           L.ptr(slab), rows, L.ptr(lse), L.ptr(lab), X.ZP_SCALE, None, None, None, None, code,
           L.stream())
    gW, gb = _slab_parts(slab, C)
    _check_pair(tag, gW, gw_bf16 if bf else gw_pair)
    _check_colsum(tag, gb, case.p)


# ---------------------------------------------------------------------------------------------
# regnn_type_project through ops.type_project_prescale
@SGN
@DTYPE
@pytest.mark.parametrize("rows", X.PROJ_ROWS)
@pytest.mark.parametrize("K", X.PROJ_K)
def test_type_project_products(K, rows, dtype, sgn):
    """h = x W^T + b without scale or dropout, keep_h: K of 2, 4 (100: a ragged last chunk, the
    per-element loads), 4 and 8 k-chunks; fp32 x: the six-product body, h per element against
    bound; bf16 x: the three-product body, h stored in bf16: w0 x0 and w1 x0 are revealed, w2 x0
    is not (see the module docstring)."""
    import types
    from regnn_hip import ops
    key = ("proj", K, rows)
    case = X.build(key, sgn)
    fp32, bf16 = case.pairs
    fc = types.SimpleNamespace(weight=_t(case.w), bias=_t(case.bias))
    if dtype == "fp32":
        h, _ = ops.type_project_prescale([fc], [_t(case.x)], None, None, keep_h=True)
        _check_pair(_tag(key, sgn), h, fp32)
        return
    hb, _ = ops.type_project_prescale([fc], [_t(case.xb, torch.bfloat16)], None, None,
                                      keep_h=True)
    _check_window(_tag(key, sgn), hb, bf16)


# ---------------------------------------------------------------------------------------------
# regnn_linear_wgrad through ops.linear_wgrad
@SGN
@DTYPE
@pytest.mark.parametrize("n", X.WGRAD_N)
@pytest.mark.parametrize("K", X.WGRAD_K)
@pytest.mark.parametrize("C", X.WGRAD_C)
def test_linear_wgrad_products(C, K, n, dtype, sgn, monkeypatch):
    """gW = g^T x, gb = colsum g; the reduction runs over the n rows, so the signed form flips
    rows (in g and x) and classes. fp32: both operands from the family, six products; bf16: both
    exact, a single product, the fp64 value up to accumulation under the same bound. C = 5: the
    ragged class loads (bf16 rows padded to a stride of 8 so the kernel takes them)."""
    from regnn_hip import ops

    def no_fallback(*_a, **_k):
        raise AssertionError("ops.linear_wgrad left regnn_linear_wgrad")
    monkeypatch.setattr(ops, "batched_wgrad", no_fallback)
    key = ("wgrad", C, K, n)
    case = X.build(key, sgn)
    fp32, bf16 = case.pairs
    if dtype == "fp32":
        gW, gb = ops.linear_wgrad(_t(case.g), _t(case.x))
        _check_pair(_tag(key, sgn), gW, fp32)
        _check_colsum(_tag(key, sgn, "/fp32"), gb, case.g)
        return
    gbuf = torch.zeros(n, 8 * ((C + 7) // 8), device=DEV, dtype=torch.bfloat16)
    gbuf[:, :C] = _t(case.gb, torch.bfloat16)
    gW, gb = ops.linear_wgrad(gbuf[:, :C], _t(case.xb, torch.bfloat16))
    _check_pair(_tag(key, sgn), gW, bf16)
    _check_colsum(_tag(key, sgn, "/bf16"), gb, case.gb)
