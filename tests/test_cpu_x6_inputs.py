"""The operands of tests/test_gpu_x6_products.py do what that file relies on, for every operand
pair it builds (same table, generator calls, seeds and shapes: _x6_ref.CASES): the planted
operands split into three nonzero one-signed bf16 parts that sum to them exactly; the kernel
body's full product set, emulated in fp64, is within 0.1 bound of the fp64 product at every
element; and every single-product mutant the pair claims to reveal (a product removed, or paired
with the wrong part) is off by >= 3 bound at every element. Printed per pair: the full set's
maximum and each mutant's minimum, as multiples of bound (pytest -s)."""
import numpy as np
import pytest

import _x6_ref as X


def _check_family(x, name):
    x0, x1, x2 = X.split3(x)
    assert (x0 != 0).all() and (x1 != 0).all() and (x2 != 0).all(), name
    s = np.sign(x)
    assert (np.sign(x0) == s).all() and (np.sign(x1) == s).all() and (np.sign(x2) == s).all(), name
    assert (x0.astype(np.float64) + x1.astype(np.float64) + x2.astype(np.float64) ==
            x.astype(np.float64)).all(), name


def _check_bf16(x, name):
    x0, x1, x2 = X.split3(x)
    assert (x0 == x).all() and (x != 0).all() and not x1.any() and not x2.any(), name


@pytest.mark.parametrize("sgn", [0, 1], ids=["plain", "signed"])
@pytest.mark.parametrize("key", X.CASES, ids=X.case_id)
def test_case_operands_reveal_each_product(key, sgn):
    case = X.build(key, sgn)
    for pr in case.pairs:
        tag = f"{X.case_id(key)}/{'signed' if sgn else 'plain'}/{pr.name}"
        # parts: a planted operand holds all three, a bf16-exact one only the first
        a_parts = {i for i, _ in pr.full}
        b_parts = {j for _, j in pr.full}
        if "a" in pr.planted:
            (_check_family if a_parts == {0, 1, 2} else _check_bf16)(pr.a, tag + " a")
        if "b" in pr.planted:
            (_check_family if b_parts == {0, 1, 2} else _check_bf16)(pr.b, tag + " b")
        ref, bnd = pr.exact(), pr.bound()
        assert (bnd > 0).all(), tag
        full = np.abs(X.emulate(pr.a, pr.b, pr.full) + (0 if pr.bias is None else
                                                        pr.bias.astype(np.float64)) - ref) / bnd
        line = [f"X6IN {tag} [{pr.body}] full max {full.max():.4f}"]
        assert (full <= 0.1).all(), (tag, float(full.max()))
        for name, prods in X.mutants(pr.full).items():
            err = np.abs(X.emulate(pr.a, pr.b, prods) + (0 if pr.bias is None else
                                                         pr.bias.astype(np.float64)) - ref) / bnd
            rev = name in pr.reveals
            line.append(f"{name}{'' if rev else ' (not claimed)'} min {err.min():.3g}")
            if rev:
                assert (err >= 3.0).all(), (tag, name, float(err.min()))
        print("; ".join(line))
        if pr.bf16_out:
            _check_bf16_window(pr, tag)


def _check_bf16_window(pr, tag):
    """a result a kernel stores in bf16 is held to _x6_ref.bf16_window, not to bound: the full
    product set passes it at every element; a lost first-order product moves the fp32 value by
    0.4 to 1 bf16 ulp, so at least a quarter of the elements leave the window (asserted); a
    second-order one leaves it only next to a rounding tie (printed, not relied on)."""
    lo, hi = X.bf16_window(pr.exact(), pr.bound())
    bias = 0 if pr.bias is None else pr.bias.astype(np.float64)

    def outside(prods):
        v = X.bf16_rne((X.emulate(pr.a, pr.b, prods) + bias).astype(np.float32))
        return int((~((v >= lo) & (v <= hi))).sum())
    assert outside(pr.full) == 0, tag
    line = [f"X6IN {tag} [{pr.body}] stored in bf16, elements outside the window of {lo.size}"]
    for name, prods in X.mutants(pr.full).items():
        n = outside(prods)
        line.append(f"{name} {n}")
        if name in X.FIRST_ORDER and name in pr.reveals:
            assert 4 * n >= lo.size, (tag, name, n)
    print("; ".join(line))


def test_planted_pairs_claim_every_mutant():
    """only the pairs with a kernel-formed p (regnn_head_bwd_z) leave mutants unclaimed, and
    those are the ones of p's remainders."""
    for key in X.CASES:
        for pr in X.build(key, 0).pairs:
            muts = X.mutants(pr.full)
            if pr.planted == "ab":
                assert pr.reveals == list(muts), (key, pr.name)
            else:
                assert key[0] == "head_bwd_z"
                assert set(pr.reveals) == set(muts) & set(X.A_GENERIC), (key, pr.name)


def test_bf16_rne_ties_and_window():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20,
                  -1.0 - 2.0 ** -8], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0], dtype=np.float32)
    assert (X.bf16_rne(x) == want).all()
    lo, hi = X.bf16_window(np.array([1.0 + 2.0 ** -8]), np.array([1e-6]))
    assert lo[0] == 1.0 and hi[0] == np.float32(1.0 + 2.0 ** -7)
    lo, hi = X.bf16_window(np.array([1.0 + 2.0 ** -9]), np.array([1e-6]))
    assert lo[0] == 1.0 and hi[0] == 1.0
