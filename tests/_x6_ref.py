"""Operands that tell a six-product bf16 split ("bf16x6") from a lesser one, and the table of
cases the bf16x6 kernels are tested on (tests/test_cpu_x6_inputs.py proves the operands reveal a
missing or mis-paired product, tests/test_gpu_x6_products.py runs the kernels on them).

The kernels split every fp32 operand x = x0 + x1 + x2 into three bf16 parts (round to nearest
even, remainders formed in fp32) and accumulate the six products a_i b_j with i + j <= 2 in fp32.
family() draws operands whose three parts are all present, positive and each near the largest
its predecessor allows, so the smallest second-order product is ~7e-6 of the full one: with one
sign per output element a lost product moves every element by > 3 x the project's GEMM
tolerance 2e-6 * sum_k |a||b| (tests/test_gpu_gemm.py), which random-sign operands average away.

Numpy only: no GPU, no torch."""
import itertools
import types

import numpy as np

SIX = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]
# b exact in bf16 (its parts 1 and 2 are zero): the three-product bodies; a exact: the mirror
B_EXACT = [(0, 0), (1, 0), (2, 0)]
A_EXACT = [(0, 0), (0, 1), (0, 2)]
ONE = [(0, 0)]
REPAIRS = [((2, 0), (2, 1)), ((1, 1), (1, 2)), ((0, 2), (2, 2)), ((0, 1), (1, 1))]


def bf16_rne(x):
    """x (fp32) rounded to the nearest bf16 (ties to even), returned as fp32: the kernels' f2bf."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """the kernels' split3: (x0, x1, x2), remainders in fp32."""
    x = np.asarray(x, dtype=np.float32)
    x0 = bf16_rne(x)
    r = (x - x0).astype(np.float32)
    x1 = bf16_rne(r)
    x2 = bf16_rne((r - x1).astype(np.float32))
    return x0, x1, x2


def emulate(a, b, products):
    """sum over (i, j) in products of a_i @ b_j in fp64 (a product listed twice counts twice)."""
    pa = [p.astype(np.float64) for p in split3(a)]
    pb = [p.astype(np.float64) for p in split3(b)]
    out = np.zeros((a.shape[0], b.shape[1]), dtype=np.float64)
    for i, j in products:
        out += pa[i] @ pb[j]
    return out


def family(rng, shape):
    """(m0 + m1 / 256 + m2 / 65536) 2^e, m0 in [128, 136], m1 in [104, 127], m2 in [56, 63],
    e in [-3, 2]: 24 bits, exact in fp32; the bf16 parts are exactly the three terms."""
    m0 = rng.integers(128, 137, size=shape)
    m1 = rng.integers(104, 128, size=shape)
    m2 = rng.integers(56, 64, size=shape)
    e = rng.integers(-3, 3, size=shape)
    v = (m0 + m1 / 256.0 + m2 / 65536.0) * np.exp2(e.astype(np.float64))
    out = v.astype(np.float32)
    assert (out.astype(np.float64) == v).all()
    return out


def bf16_family(rng, shape):
    return bf16_rne(family(rng, shape))


def signs(rng, n):
    return (1.0 - 2.0 * rng.integers(0, 2, size=n)).astype(np.float32)


def signed(a, b, rng):
    """a [M, K], b [K, N] with the sign of reduction index k flipped in both and whole rows of a
    flipped: every partial product of an output element keeps one sign."""
    sk, sr = signs(rng, a.shape[1]), signs(rng, a.shape[0])
    return a * sr[:, None] * sk[None, :], b * sk[:, None]


def bound(a, b, bias=None):
    """the GEMM tolerance of tests/test_gpu_gemm.py per element: 2e-6 (|a| @ |b| + |bias|)."""
    m = np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))
    if bias is not None:
        m = m + np.abs(np.asarray(bias, dtype=np.float64))
    return 2e-6 * m


def exact(a, b, bias=None):
    r = a.astype(np.float64) @ b.astype(np.float64)
    return r if bias is None else r + np.asarray(bias, dtype=np.float64)


def mutants(full):
    """{name: product list} of every single-product mutant of the set `full`: each product
    removed, and each re-pairing of REPAIRS whose source the set holds."""
    out = {}
    for p in full:
        out["drop%s" % (p,)] = [x for x in full if x != p]
    for src, dst in REPAIRS:
        if src in full:
            out["%s->%s" % (src, dst)] = [x for x in full if x != src] + [dst]
    return out


def bf16_window(ref, bnd):
    """[lo, hi] (fp32 values exact in bf16): what a bf16-stored result may be when the fp32 value
    it was rounded from lies within bnd of ref (round to nearest even is monotone)."""
    lo = np.nextafter((ref - bnd).astype(np.float32), np.float32(-np.inf))
    hi = np.nextafter((ref + bnd).astype(np.float32), np.float32(np.inf))
    return bf16_rne(lo), bf16_rne(hi)


class Pair:
    """one product a @ b (+ bias) a case checks: `full` is the product set of the kernel body
    that computes it, (i, j) = (part of a, part of b); `planted` says which operands come from
    the family (the other is generic: only the products of its part 0 can be revealed);
    `reveals` the mutants whose error is >= 3 bound at every element (None: all of them);
    `bf16_out`: a kernel stores this result in bf16, where it is held to bf16_window."""

    def __init__(self, name, a, b, bias=None, full=SIX, planted="ab", reveals=None, body="",
                 bf16_out=False):
        self.name, self.a, self.b, self.bias, self.full = name, a, b, bias, list(full)
        self.planted, self.body, self.bf16_out = planted, body, bf16_out
        muts = mutants(self.full)
        self.reveals = list(muts) if reveals is None else [m for m in muts if m in reveals]

    def exact(self):
        return exact(self.a, self.b, self.bias)

    def bound(self):
        return bound(self.a, self.b, self.bias)


# the mutants that lose or mis-pair a first-order product (or the leading one)
FIRST_ORDER = ["drop(0, 0)", "drop(0, 1)", "drop(1, 0)", "(0, 1)->(1, 1)"]

# mutants a pair with a generic (unplanted) `a` reveals: the products of its part 0, and the
# re-pairings that replace one of them (a generic remainder has random sign and size)
A_GENERIC = ["drop(0, 0)", "drop(0, 1)", "drop(0, 2)", "(0, 2)->(2, 2)", "(0, 1)->(1, 1)"]

# ---------------------------------------------------------------------------------------------
# the case table: one builder per kernel entry, keyed (kind, *shape); build(key, sgn) returns a
# namespace of the operands as the kernel takes them (numpy, fp32) and the Pairs to check.
GEMM_SHAPES = [(16, 16, 32), (130, 132, 64), (150, 200, 96), (65, 35, 33), (130, 132, 256)]
GEMM_LIVE = (200, 132, 64, 70)               # M, N, K, m_live
GEMM_ABI = (130, 132, 96)                    # regnn_gemm_x6 by the ABI: ld, offset, beta
GEMM_KLIVE = (130, 132, 96, 40)              # ... and k_live
HEAD_ROWS, HEAD_C = [1, 17, 300], [3, 33, 349, 368]
BWD_N, BWD_C = [5, 300], [33, 349]
PROJ_K, PROJ_ROWS = [64, 100, 128, 256], [1, 50]
WGRAD_C, WGRAD_K, WGRAD_N = [5, 64], [64, 128, 256], [33, 300]
ZP_SCALE = 0.25


def _rng(key, sgn):
    h = 0
    for v in key:
        for ch in str(v):
            h = (h * 131 + ord(ch)) % (1 << 31)
    return np.random.default_rng([h, int(sgn)])


def _gemm(key, sgn):
    M, N, K = key[1:4]
    rng = _rng(key, sgn)
    a, b = family(rng, (M, K)), family(rng, (K, N))
    if sgn:
        a, b = signed(a, b, rng)
    c = types.SimpleNamespace(a=a, b=b, c0=None)
    la, lb = a, b
    if key[0] == "gemm_live":                 # rows >= m_live of op(a) are zero
        a[key[4]:] = 0
        la = a[:key[4]]
    if key[0] == "gemm_klive":                # both operands zero past k_live
        a[:, key[4]:] = 0
        b[key[4]:] = 0
        la, lb = a[:, :key[4]], b[:key[4]]
    if key[0] == "gemm_abi":
        c.c0 = family(rng, (M, N)) * (signs(rng, M)[:, None] if sgn else 1.0)
    c.pairs = [Pair("c", la, lb, body="gemm_x6_kernel")]
    return c


def _head_fwd(key, sgn):
    """logits = h W^T + b: h [rows, 64] fp32 (six products) and bf16 (hb: the three-product
    body), W [C, 64], bias [C]."""
    rows, C = key[1:3]
    rng = _rng(key, sgn)
    h, hb = family(rng, (rows, 64)), bf16_family(rng, (rows, 64))
    w, bias = family(rng, (C, 64)), family(rng, (C,))
    if sgn:
        sk, sr = signs(rng, 64), signs(rng, rows)
        h, hb = h * sr[:, None] * sk, hb * sr[:, None] * sk
        w = w * sk
    wt = np.ascontiguousarray(w.T)
    return types.SimpleNamespace(h=h, hb=hb, w=w, bias=bias, pairs=[
        Pair("logits", h, wt, bias, body="head_fwd_x6_kernel<float>"),
        Pair("logits_bf16", hb, wt, bias, full=A_EXACT, body="head_fwd_x6_kernel<bf16>")])


def _head_bwd(key, sgn):
    """gh = p W, gW = p^T h, gb = colsum p with a planted p [n, C]."""
    n, C = key[1:3]
    rng = _rng(key, sgn)
    p, w, h = family(rng, (n, C)), family(rng, (C, 64)), family(rng, (n, 64))
    if sgn:                                   # classes in p and W, rows in p and h
        sc, sn = signs(rng, C), signs(rng, n)
        p, w, h = p * sn[:, None] * sc, w * sc[:, None], h * sn[:, None]
    return types.SimpleNamespace(p=p, w=w, h=h, pairs=[
        Pair("gh", p, w, body="head_gh_x6_kernel"),
        Pair("gW", np.ascontiguousarray(p.T), h, body="wgrad_x6_kernel<float, float>")])


def zp_formula(z, lse, labels, scale):
    """the fp32 p regnn_head_bwd_z forms: scale (exp(z - lse) - [class == label])."""
    p = np.exp(z.astype(np.float64) - lse.astype(np.float64)[:, None])
    p[np.arange(len(labels)), labels] -= 1.0
    return (scale * p).astype(np.float32)


def _head_bwd_z(key, sgn):
    """regnn_head_bwd_z: p is formed in the kernel from z, lse and the labels, so only W (gh)
    and h (the slab) are planted. lse is an input of the entry: the test passes a value below
    every logit of the row, so exp(z - lse) > 1.6 and p is positive at the label too (one sign
    per output element; the kernel's formula does not care). sgn flips whole output columns."""
    n, C = key[1:3]
    rng = _rng(key, sgn)
    z = rng.standard_normal((n, C)).astype(np.float32)
    lse = (z.min(axis=1) - 0.5).astype(np.float32)
    labels = rng.integers(0, C, size=n)
    p = zp_formula(z, lse, labels, ZP_SCALE)
    w, h, hb = family(rng, (C, 64)), family(rng, (n, 64)), bf16_family(rng, (n, 64))
    if sgn:
        s = signs(rng, 64)
        w, h, hb = w * s, h * s, hb * s
    pt = np.ascontiguousarray(p.T)
    return types.SimpleNamespace(z=z, lse=lse, labels=labels, p=p, w=w, h=h, hb=hb, pairs=[
        Pair("gh", p, w, planted="b", reveals=A_GENERIC, body="head_gh_x6_kernel<ZP>",
             bf16_out=True),                  # (with bf16 rows; fp32 rows: held to bound)
        Pair("gW", pt, h, planted="b", reveals=A_GENERIC, body="wgrad_x6_kernel<float, float, ZP>"),
        Pair("gW_bf16", pt, hb, full=B_EXACT, planted="b", reveals=A_GENERIC,
             body="wgrad_x6_kernel<float, bf16, ZP>")])


def _proj(key, sgn):
    """h = x W^T + b, x [rows, K] fp32 and bf16 (xb), W [64, K]."""
    K, rows = key[1:3]
    rng = _rng(key, sgn)
    x, xb = family(rng, (rows, K)), bf16_family(rng, (rows, K))
    w, bias = family(rng, (64, K)), family(rng, (64,))
    if sgn:
        sk, sr = signs(rng, K), signs(rng, rows)
        x, xb, w = x * sr[:, None] * sk, xb * sr[:, None] * sk, w * sk
    wt = np.ascontiguousarray(w.T)
    return types.SimpleNamespace(x=x, xb=xb, w=w, bias=bias, pairs=[
        Pair("h", x, wt, bias, body="type_project_kernel<float>"),
        Pair("h_bf16", xb, wt, bias, full=A_EXACT, body="type_project_kernel<bf16>",
             bf16_out=True)])


def _wgrad(key, sgn):
    """gW = g^T x, gb = colsum g over n rows (the reduction index), fp32 and bf16 operands."""
    C, K, n = key[1:4]
    rng = _rng(key, sgn)
    g, x = family(rng, (n, C)), family(rng, (n, K))
    gb, xb = bf16_family(rng, (n, C)), bf16_family(rng, (n, K))
    if sgn:                                   # rows in both, classes in g
        sn, sc = signs(rng, n), signs(rng, C)
        g, gb = g * sn[:, None] * sc, gb * sn[:, None] * sc
        x, xb = x * sn[:, None], xb * sn[:, None]
    return types.SimpleNamespace(g=g, x=x, gb=gb, xb=xb, pairs=[
        Pair("gW", np.ascontiguousarray(g.T), x, body="linear_wgrad_kernel<float>"),
        Pair("gW_bf16", np.ascontiguousarray(gb.T), xb, full=ONE,
             body="linear_wgrad_kernel<bf16>")])


_BUILDERS = {"gemm": _gemm, "gemm_live": _gemm, "gemm_abi": _gemm, "gemm_klive": _gemm,
             "head_fwd": _head_fwd, "head_bwd": _head_bwd, "head_bwd_z": _head_bwd_z,
             "proj": _proj, "wgrad": _wgrad}

CASES = ([("gemm",) + s for s in GEMM_SHAPES] + [("gemm_live",) + GEMM_LIVE,
                                                 ("gemm_abi",) + GEMM_ABI,
                                                 ("gemm_klive",) + GEMM_KLIVE]
         + [("head_fwd", r, c) for r, c in itertools.product(HEAD_ROWS, HEAD_C)]
         + [("head_bwd", n, c) for n, c in itertools.product(BWD_N, BWD_C)]
         + [("head_bwd_z", n, c) for n, c in itertools.product(BWD_N, BWD_C)]
         + [("proj", k, r) for k, r in itertools.product(PROJ_K, PROJ_ROWS)]
         + [("wgrad", c, k, n) for c, k, n in itertools.product(WGRAD_C, WGRAD_K, WGRAD_N)])


def build(key, sgn):
    assert key in CASES, key
    return _BUILDERS[key[0]](key, bool(sgn))


def case_id(key):
    return "-".join(str(v) for v in key)
