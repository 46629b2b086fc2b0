"""The wide NS model's tail operators alone against fp64: ops.wide_ln_act (regnn_wide_ln_fwd /
_bwd), ops.softmax_xent and ops.ns_lin_xent (xent_rows / xent_sum / xent_bwd / ns_xent_fwd /
xent_bwd_colsum of re_ns.hip) and ops.rel_tabs -- so a failure of tests/test_gpu_nsmod_matrix.py
in one of them reads without the model around it.

Metric: _nsm_ref.own_scale_error (no floor; an element whose reference is exactly zero must be
exactly zero), column sums per element against the sum of their terms' absolute values, bound
_nsm_ref.TOL = 1e-5. Every input is built on the host from a numpy generator, so the conditions
the inputs must meet (below) do not depend on a device."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _nsm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LN_EPS = 1e-5
STATE = [123, 2, 0, 9, 0, 0, 0, 0]
LAYER = 1
ULP_1E3 = 2.0 ** -14                           # fp32 spacing in [512, 1024)


# ---------------------------------------------------------------------------------------------
# ops.wide_ln_act
# ---------------------------------------------------------------------------------------------
def ln_rows(H):
    """512 blocks of 256 / LPR rows + 3: the backward's clamped grid (regnn_wide_ln_slab_rows)
    strides once more over a ragged last group."""
    lpr = 64 if H >= 256 else H // 4
    return 512 * (256 // lpr) + 3


def _grid(a, bits):
    """values on a 2^-bits grid: sums and differences of a few of them are exact in fp32"""
    return np.round(a * 2.0 ** bits) / 2.0 ** bits


@functools.lru_cache(maxsize=None)
def ln_inputs(H, res, rs, bias, p):
    """host inputs of one configuration. Planted rows (n // 3 + ...):
    r_const: a = rs x + bias + res is exactly 2 in every column (bias and that row of res lie on
      a 2^-8 grid, rs = 0.5): variance 0, rstd = 1 / sqrt(eps); its gy is scaled by sqrt(eps) / 4 so
      its gradient row does not set the tensor's scale;
    r_off: x = 1e3 + s, 0.5 <= |s| <= 1.5 (rs = 1, res = 0 there);
    r_zero: rs = 0 (with rs): gx exactly 0.
    gy is zero wherever the fp64 LayerNorm output lies within 1e-4 (1e-2 on r_off) of relu's
    kink: there an fp32 rounding decides the branch, and the gradient of either branch is right."""
    n = ln_rows(H)
    rng = np.random.default_rng(7000 + H + 10 * int(res) + 20 * int(rs) + 40 * int(bias))
    x = rng.standard_normal((n, H)).astype(np.float32)
    s = (rng.random(n) + 0.5).astype(np.float32) if rs else None
    b = _grid(rng.standard_normal(H), 8).astype(np.float32) if bias else None
    r = rng.standard_normal((n, H)).astype(np.float32) if res else None
    gamma = (1 + 0.2 * rng.standard_normal(H)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(H)).astype(np.float32)
    gy = rng.standard_normal((n, H)).astype(np.float32)
    r_const, r_off, r_zero = n // 3, n // 3 + 1, n // 3 + 2
    bb = b if bias else np.zeros(H, np.float32)
    if res:
        r[r_const] = _grid(r[r_const], 8)
        r[r_off] = 0
    rc = r[r_const] if res else np.zeros(H, np.float32)
    if rs:
        s[r_const], s[r_off], s[r_zero] = 0.5, 1.0, 0.0
    x[r_const] = (2.0 - bb - rc) * (2.0 if rs else 1.0)
    spread = (0.5 + rng.random(H)) * np.where(rng.random(H) < 0.5, -1.0, 1.0)
    x[r_off] = (1e3 + spread).astype(np.float32)
    gy[r_const] *= np.float32(np.sqrt(LN_EPS) / 4)
    keep16 = int(round((1 - p) * 65536))
    mask = (R.O.dropout_mask(R.nsm_seed(STATE, LAYER), n, H, 4, keep16) / (keep16 / 65536)
            if p > 0 else np.ones((n, H)))
    d = dict(n=n, H=H, x=x, rs=s, bias=b, res=r, gamma=gamma, beta=beta, gy=gy, mask=mask, p=p,
             r_const=r_const, r_off=r_off, r_zero=r_zero if rs else None)
    pre = ln_reference(d, None)["pre"]
    near = np.abs(pre) < 1e-4
    near[r_off] = np.abs(pre[r_off]) < 1e-2
    gy[near] = 0
    a_const = (s[r_const] if rs else 1.0) * x[r_const].astype(np.float64) + bb + rc
    assert np.all(a_const == 2.0)
    return d


def ln_reference(d, live):
    """fp64 autograd of dropout(relu(LayerNorm(rs x + bias + res))) (the LayerNorm written out:
    _nsm_ref._layer_norm) with gy zero from row min(n, live) on -> y, pre (LayerNorm's output),
    a, rstd, gx, gres and the three column gradients with their sums of absolute terms (the
    bias gradient's term d a is itself a cancelling sum of three products: s_bias below)."""
    n, H = d["n"], d["H"]
    rows = n if live is None else min(n, live)
    t = lambda v: None if v is None else torch.from_numpy(np.asarray(v, np.float64))  # noqa: E731
    x = t(d["x"]).requires_grad_()
    bias = t(d["bias"]) if d["bias"] is not None else None
    res = t(d["res"]).requires_grad_() if d["res"] is not None else None
    ln = types.SimpleNamespace(eps=LN_EPS, weight=t(d["gamma"]).requires_grad_(),
                               bias=t(d["beta"]).requires_grad_())
    a = x * t(d["rs"]).view(-1, 1) if d["rs"] is not None else x * 1.0
    if bias is not None:
        bias.requires_grad_()
        a = a + bias
    if res is not None:
        a = a + res
    a.retain_grad()
    pre = R._layer_norm(a, ln)
    pre.retain_grad()
    y = torch.relu(pre) * t(d["mask"])
    gy = t(d["gy"]).clone()
    gy[rows:] = 0
    y.backward(gy)
    ad = a.detach()
    mu = ad.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((ad - mu) ** 2).mean(1, keepdim=True) + LN_EPS)
    xhat = (ad - mu) * rstd
    # d a = rstd (g - mean g - xhat mean(g xhat)), g = gy' gamma: three products that cancel; its
    # column sum is judged against the sum with every product replaced by its absolute value
    g = pre.grad * ln.weight.detach()
    s_bias = (rstd * (g.abs() + g.mean(1, keepdim=True).abs()
                      + xhat.abs() * (g * xhat).mean(1, keepdim=True).abs())).sum(0)
    out = dict(y=y.detach().numpy(), pre=pre.detach().numpy(), a=ad.numpy(),
               rstd=rstd.view(-1).numpy(), gx=x.grad.numpy(),
               gres=None if res is None else res.grad.numpy(),
               g_gamma=ln.weight.grad.numpy(), s_gamma=(pre.grad * xhat).abs().sum(0).numpy(),
               g_beta=ln.bias.grad.numpy(), s_beta=pre.grad.abs().sum(0).numpy(),
               g_bias=None if bias is None else bias.grad.numpy(),
               s_bias=s_bias.numpy(), ga=a.grad.numpy(), gpre=pre.grad.numpy(),
               xhat=xhat.numpy(), rows=rows)
    return out


def offset_row_bounds(d, ref):
    """what fp32 can hold on the planted offset row, from the number format alone.

    a = 1e3 + s is rounded to fp32's spacing ulp(1e3) = 2^-14 there: with at most two roundings
    forming a (the fma, the residual add) and one in the row mean, xhat = (a - mean) rstd is off
    by d_x <= 3 ulp(1e3) rstd, whatever the kernel. y = relu(gamma xhat + beta) m then moves by at
    most max|gamma m| d_x, which the issue judges on the row's own max|a| (own-scale of the tensor
    the rounding happens on): |y - ref| <= TOL max|a_row|; the derived figure (2e-4 at rstd 1.2)
    lies far inside it. ga = rstd (g - mean g - xhat mean(g xhat)), g = gy' gamma, moves by at most
    rstd d_x (|mean(g xhat)| + mean|g|): that, on top of TOL of the tensor's scale, bounds gx
    and gres on this row."""
    o = d["r_off"]
    rstd = float(ref["rstd"][o])
    dx = 3 * ULP_1E3 * rstd
    g = ref["gpre"][o] * d["gamma"].astype(np.float64)
    slack = rstd * dx * (abs(float((g * ref["xhat"][o]).mean())) + float(np.abs(g).mean()))
    return R.TOL * float(np.abs(ref["a"][o]).max()), slack


def _max_err(got, ref):
    """max |got - ref| / max |ref| (0 for an empty or all-zero reference that got matches)"""
    if not ref.size:
        return 0.0
    assert np.all(np.isfinite(got))
    e, s_ = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    return e / s_ if s_ > 0 else (0.0 if e == 0 else float("inf"))


LN_CONFIGS = [(False, True, True, 0.5), (True, True, True, 0.0), (False, False, False, 0.0),
              (True, False, True, 0.5), (False, True, False, 0.5)]


@pytest.mark.parametrize("res,rs,bias,p", LN_CONFIGS)
@pytest.mark.parametrize("H", [64, 128, 256, 512, 1024])
def test_wide_ln_act_matches_fp64(H, res, rs, bias, p):
    """n = 512 (256 / LPR) + 3 rows (the backward's 512-block clamp loops, ragged), live in None,
    0, 1, n - 1, n, n + 5: rows below min(n, live) are compared, gx past them is exactly zero
    (with `res` the operator drops `live`, as its docstring says: every row is then formed and
    compared). Planted rows and the offset row's bound: ln_inputs, offset_row_bounds."""
    from regnn_hip import ops
    d = ln_inputs(H, res, rs, bias, p)
    n, o = d["n"], d["r_off"]
    dev = lambda v: None if v is None else torch.from_numpy(v).to(DEV)  # noqa: E731
    ln = torch.nn.LayerNorm(H).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(dev(d["gamma"]))
        ln.bias.copy_(dev(d["beta"]))
    state = torch.tensor(STATE, dtype=torch.int64, device=DEV)
    worst, refs = {}, {}
    for live in (None, 0, 1, n - 1, n, n + 5):
        rows = n if (res or live is None) else min(n, live)
        if rows not in refs:
            refs[rows] = ln_reference(d, rows)
        ref = refs[rows]
        x = dev(d["x"]).requires_grad_()
        b = dev(d["bias"]).requires_grad_() if bias else None
        r = dev(d["res"]).requires_grad_() if res else None
        for q in (ln.weight, ln.bias):
            q.grad = None
        lv = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
        y = ops.wide_ln_act(x, b, ln, p, state, LAYER, rs=dev(d["rs"]), res=r, live=lv)
        y.backward(dev(d["gy"]))
        torch.cuda.synchronize()
        got = dict(y=y.detach(), gx=x.grad, gres=r.grad if res else None)
        got = {k: None if v is None else v.cpu().double().numpy() for k, v in got.items()}
        y_bound, g_slack = offset_row_bounds(d, ref)
        body = np.ones(n, bool)
        body[rows:] = False
        errs = {}
        if rows > o:
            body[o] = False
            errs["y[offset row]/max|a|"] = R.TOL * float(np.abs(got["y"][o] - ref["y"][o]).max()) / y_bound
        # (relu's zeros are no structural zeros: an fp32 rounding next to the kink may leave
        # 1e-7 where the reference holds 0; the dropped elements are)
        assert not got["y"][:rows][d["mask"][:rows] == 0].any()
        errs["y"] = _max_err(got["y"][body], ref["y"][body])
        for k in ("gx", "gres"):
            if got[k] is None:
                continue
            assert not got[k][rows:].any(), f"{k} past the live count"
            errs[k] = R.own_scale_error(got[k][body], ref[k][body])
            if rows > o:
                scale = float(np.abs(ref[k]).max())
                e = float(np.abs(got[k][o] - ref[k][o]).max())
                errs[k + "[offset row]"] = R.TOL * e / (R.TOL * scale + g_slack)
        cols = [("g_gamma", ln.weight.grad), ("g_beta", ln.bias.grad)] + \
            ([("g_bias", b.grad)] if bias else [])
        for k, g in cols:
            errs[k] = R.own_scale_error(g.cpu().double().numpy(), ref[k], ref["s" + k[1:]])
        for k, e in errs.items():
            print(f"WIDE_LN H={H} res={res} rs={rs} bias={bias} p={p} live={live} {k}: {e:.3e}")
            worst[k] = max(worst.get(k, 0.0), e)
        if rows > d["r_const"]:
            assert np.all(np.isfinite(got["gx"][d["r_const"]]))
        if d["r_zero"] is not None and rows > d["r_zero"]:
            assert not got["gx"][d["r_zero"]].any()
    bad = {k: e for k, e in worst.items() if not e <= R.TOL}
    assert not bad, f"own-scale error past {R.TOL:g}: {bad}"


# ---------------------------------------------------------------------------------------------
# ops.softmax_xent / ops.ns_lin_xent
# ---------------------------------------------------------------------------------------------
XENT_C = [1, 5, 63, 64, 65, 349]
XENT_B = [1, 3, 257, 1030, 2053]


@functools.lru_cache(maxsize=None)
def xent_inputs(B, C):
    """logits on a 2^-10 grid (so z = x + b is exact in fp32): randn * 3, row offsets of +80 / -80
    / 0 by row mod 3 (exp overflows, or underflows to 0, without the max subtraction); every 5th row
    of offset <= 0 has one logit 60 above the rest; on every 7th row of offset +80 the labelled
    logit is 100 below the maximum. A label never sits on a class of probability > 1/2: 1 - p_y
    = -gz_y n would cancel in fp32 and the row's own scale with it (C = 1 has no other class: its
    loss and gradient are exactly zero)."""
    rng = np.random.default_rng(9000 + 7 * B + C)
    z = _grid(rng.standard_normal((B, C)) * 3, 10)
    off = np.array([80.0, -80.0, 0.0])[np.arange(B) % 3]
    z += off[:, None]
    y = rng.integers(C, size=B)
    for r in range(B):
        if off[r] <= 0 and r % 5 == 0:
            z[r, rng.integers(C)] = z[r].max() + 60
        if off[r] > 0 and r % 7 == 0 and C > 1:
            z[r, y[r]] = z[r].max() - 100
    if C > 1:
        p = torch.from_numpy(z).softmax(1).numpy()
        hot = p[np.arange(B), y] > 0.5
        y[hot] = (y[hot] + 1) % C
        assert np.all(p[np.arange(B), y] <= 0.5)
    b = _grid(rng.standard_normal(C), 6)
    x = z - b
    assert np.array_equal((x.astype(np.float32).astype(np.float64) + b.astype(np.float32)), z)
    return dict(z=z.astype(np.float32), x=x.astype(np.float32), b=b.astype(np.float32),
                y=y.astype(np.int64))


def xent_reference(z, y, C):
    """fp64 log_softmax + nll_loss, mean over the rows whose label lies in [0, C) -> loss, gz,
    gb and gb's sum of absolute terms."""
    z64 = torch.from_numpy(z.astype(np.float64)).requires_grad_()
    yt = torch.from_numpy(y).clone()
    on = (yt >= 0) & (yt < C)
    yt[~on] = -100
    if not on.any():
        return dict(loss=float("nan"), gz=np.zeros(z.shape), gb=np.zeros(C), sb=np.zeros(C), on=on.numpy())
    loss = F.nll_loss(F.log_softmax(z64, 1), yt, ignore_index=-100)
    loss.backward()
    gz = z64.grad.numpy()
    return dict(loss=float(loss.detach()), gz=gz, gb=gz.sum(0), sb=np.abs(gz).sum(0), on=on.numpy())


def _xent_errs(tag, loss, gz, gb, ref):
    errs = {}
    if np.isnan(ref["loss"]):
        assert np.isnan(loss), f"{tag}: every row ignored: the documented NaN, got {loss}"
    else:
        errs["loss"] = R.own_scale_error(loss, ref["loss"])
    assert not gz[~ref["on"]].any(), f"{tag}: gz on an ignored row"
    if not np.isnan(ref["loss"]):
        errs["gz[per row]"] = max([R.own_scale_error(gz[r], ref["gz"][r])
                                   for r in range(gz.shape[0])], default=0.0)
        if gb is not None:
            errs["gb"] = R.own_scale_error(gb, ref["gb"], ref["sb"])
    for k, e in errs.items():
        print(f"XENT {tag} {k}: {e:.3e}")
    return errs


def _run_softmax_xent(z, y):
    from regnn_hip import ops
    zt = torch.from_numpy(z).to(DEV).requires_grad_()
    loss = ops.softmax_xent(zt, torch.from_numpy(y).to(DEV))
    if zt.shape[0]:
        loss.backward()
    torch.cuda.synchronize()
    return float(loss), zt.grad.cpu().double().numpy(), None


def _run_ns_lin_xent(d, y, live, ticket):
    """z = x I^T + b (exact), labels through a permuted n_id, `live` targets."""
    from regnn_hip import ops
    B, C = d["z"].shape
    rng = np.random.default_rng(B + C)
    n_id = rng.permutation(B + 11)[:B].astype(np.int32)
    labels = np.full(B + 11, 3, np.int64)
    labels[n_id] = y
    x = torch.from_numpy(d["x"]).to(DEV).requires_grad_()
    w = torch.eye(C, device=DEV).requires_grad_()
    b = torch.from_numpy(d["b"]).to(DEV).requires_grad_()
    sizes = torch.zeros(16, dtype=torch.int32, device=DEV)
    sizes[0] = live
    loss = ops.ns_lin_xent(x, w, b, torch.from_numpy(n_id).to(DEV), sizes,
                           torch.from_numpy(labels).to(DEV), ticket)
    loss.backward()
    torch.cuda.synchronize()
    assert int(ticket.item()) == 0, "the ticket must be back at zero"
    # W = I: gx = gz W is gz itself
    return float(loss), x.grad.cpu().double().numpy(), b.grad.cpu().double().numpy(), \
        w.grad.cpu().double().numpy()


@pytest.mark.parametrize("C", XENT_C)
@pytest.mark.parametrize("B", XENT_B)
def test_xent_matches_fp64(B, C):
    """both losses over B rows of C logits with `live` in 0, 1, B - 1, B (softmax_xent: the rows
    past it labelled -100): loss own-scale, gz own-scale per row, out_lin's bias gradient per
    element against sum_r |gz[r][c]|; the ticket back at zero."""
    d = xent_inputs(B, C)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = {}
    for live in sorted({0, 1, B - 1, B}):
        y = d["y"].copy()
        y[live:] = -100
        ref = xent_reference(d["z"], y, C)
        for k, e in _xent_errs(f"softmax_xent B={B} C={C} live={live}",
                               *_run_softmax_xent(d["z"], y), ref).items():
            worst["softmax_xent " + k] = max(worst.get("softmax_xent " + k, 0.0), e)
        loss, gx, gb, gw = _run_ns_lin_xent(d, d["y"], live, ticket)
        errs = _xent_errs(f"ns_lin_xent B={B} C={C} live={live}", loss, gx, gb, ref)
        if not np.isnan(ref["loss"]):
            x64 = d["x"].astype(np.float64)
            errs["gw"] = R.own_scale_error(gw, ref["gz"].T @ x64, np.abs(ref["gz"]).T @ np.abs(x64))
        for k, e in errs.items():
            worst["ns_lin_xent " + k] = max(worst.get("ns_lin_xent " + k, 0.0), e)
    bad = {k: e for k, e in worst.items() if not e <= R.TOL}
    assert not bad, f"B={B} C={C}: error past {R.TOL:g}: {bad}"


@pytest.mark.parametrize("B,C", [(257, 37), (1030, 5), (19, 349)])
def test_xent_ignores_labels_outside_the_classes(B, C):
    """labels -1, -100, C and C + 7 on interior rows: loss, gz and gb equal the fp64 reference with
    those rows ignored, gz exactly zero on them (no kernel indexes z with such a label); the
    all-ignored batch keeps the documented NaN loss."""
    d = xent_inputs(B, C) if (B in XENT_B and C in XENT_C) else None
    if d is None:
        rng = np.random.default_rng(B * 1000 + C)
        z = _grid(rng.standard_normal((B, C)) * 3, 10)
        b = _grid(rng.standard_normal(C), 6)
        y = rng.integers(C, size=B)
        p = torch.from_numpy(z).softmax(1).numpy()
        hot = p[np.arange(B), y] > 0.5
        y[hot] = (y[hot] + 1) % C
        d = dict(z=z.astype(np.float32), x=(z - b).astype(np.float32), b=b.astype(np.float32),
                 y=y.astype(np.int64))
    y = d["y"].copy()
    bad_rows = {3: -1, 7: -100, B // 2: C, B // 2 + 1: C + 7, B - 2: -1}
    for r, v in bad_rows.items():
        y[r] = v
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref = xent_reference(d["z"], y, C)
    assert int(ref["on"].sum()) == B - len(bad_rows)
    errs = _xent_errs(f"softmax_xent labels B={B} C={C}", *_run_softmax_xent(d["z"], y), ref)
    loss, gx, gb, _ = _run_ns_lin_xent(d, y, B, ticket)
    errs.update({"lin " + k: e for k, e in
                 _xent_errs(f"ns_lin_xent labels B={B} C={C}", loss, gx, gb, ref).items()})
    bad = {k: e for k, e in errs.items() if not e <= R.TOL}
    assert not bad, bad
    y[:] = [-1, -100, C, C + 7][B % 4]
    y[::2] = -1
    ref = xent_reference(d["z"], y, C)
    _xent_errs("softmax_xent all ignored", *_run_softmax_xent(d["z"], y), ref)
    loss, gx, gb, _ = _run_ns_lin_xent(d, y, B, ticket)
    _xent_errs("ns_lin_xent all ignored", loss, gx, None, ref)


# ---------------------------------------------------------------------------------------------
# ops.mm with a live-row count
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("live", [0, 1, 77, 300])
@pytest.mark.parametrize("route", ["x6", "x6_live_rows_off", "torch"])
def test_mm_ignores_rows_past_the_live_count(monkeypatch, route, live):
    """a's rows from the next multiple of 128 past `live` on are unspecified (NaN here), the rows
    between zero (regnn_ns_slot_agg's contract: the x6 GEMM's last live tile reads them), and the
    incoming gradient's rows past `live` are zero, as layer 0 of the module path hands them over:
    out[:live], ga[:live] and gb = a^T g equal fp64
    over the live rows on the x6 GEMM, on x6 without its live bound (LIVE_ROWS "off") and on
    torch's product (GEMM_X6 "off"); each element against the sum of its |products|."""
    from regnn_hip import ops
    if route == "x6_live_rows_off":
        monkeypatch.setitem(ops.LIVE_ROWS, "mode", "off")
    if route == "torch":
        monkeypatch.setitem(ops.GEMM_X6, "mode", "off")
    M_, K, N = 300, 132, 128
    rng = np.random.default_rng(live)
    a = rng.standard_normal((M_, K)).astype(np.float32)
    b = rng.standard_normal((K, N)).astype(np.float32)
    g = rng.standard_normal((M_, N)).astype(np.float32)
    a[live:], g[live:] = 0.0, 0.0
    a[-(-live // 128) * 128:] = np.nan
    at = torch.from_numpy(a).to(DEV).requires_grad_()
    bt = torch.from_numpy(b).to(DEV).requires_grad_()
    out = ops.mm(at, bt, live=torch.tensor([live], dtype=torch.int32, device=DEV))
    out.backward(torch.from_numpy(g).to(DEV))
    torch.cuda.synchronize()
    a64, b64, g64 = a[:live].astype(np.float64), b.astype(np.float64), g[:live].astype(np.float64)
    checks = [("out", out.detach()[:live], a64 @ b64, np.abs(a64) @ np.abs(b64)),
              ("ga", at.grad[:live], g64 @ b64.T, np.abs(g64) @ np.abs(b64).T),
              ("gb", bt.grad, a64.T @ g64, np.abs(a64).T @ np.abs(g64))]
    for name, got, ref, scale in checks:
        e = R.own_scale_error(got.cpu().double().numpy(), ref, scale)
        print(f"MM_LIVE {route} live={live} {name}: {e:.3e}")
        assert e <= R.TOL, (name, e)


# ---------------------------------------------------------------------------------------------
# ops.rel_tabs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(1,), (256,), (5, 300, 1, 17), (0, 23)])
def test_rel_tabs_exact(sizes):
    """leaky_relu(alpha rw) per table, forward bitwise against torch's fp32, backward exactly the
    one product g alpha (or g (slope alpha)); 0.0 is planted in every non-empty table: the forward
    gives 0 on either branch and the backward takes the slope side (alpha rw > 0 is false)."""
    from regnn_hip import ops
    alpha, slope = 10.0, 0.01
    rng = np.random.default_rng(sum(sizes))
    rws = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in sizes]
    for rw in rws:
        if rw.size:
            rw[rw.size // 2] = 0.0
    gs = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    dev = [torch.from_numpy(r).to(DEV).requires_grad_() for r in rws]
    tabs = ops.rel_tabs(dev, alpha, slope)
    sum((t * torch.from_numpy(g).to(DEV)).sum() for t, g in zip(tabs, gs)).backward()
    torch.cuda.synchronize()
    for rw, g, t, q in zip(rws, gs, tabs, dev):
        want = F.leaky_relu(torch.from_numpy(rw) * alpha, slope)
        assert torch.equal(t.detach().cpu(), want)
        pos = np.float32(alpha) * rw > 0
        gw = np.where(pos, g * np.float32(alpha), g * (np.float32(slope) * np.float32(alpha)))
        assert np.array_equal(q.grad.cpu().numpy(), gw.astype(np.float32))
