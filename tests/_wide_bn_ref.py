"""numpy fp64 restatement of ops.wide_bn_act (regnn_wide_bn_fwd / _bwd, include/regnn_hip.h): the
NS model's per-layer epilogue with BatchNorm1d in training mode over the first `live` rows of a
capacity-sized block. A plain helper: no test lives here.

  a[v]  = rs[v] x[v] + bias + res[v]                                   v < live
  mean, var (biased) per column over those rows
  y[v]  = mask[v] relu(gamma (a[v] - mean) / sqrt(var + eps) + beta)   v < live;   0 past them
  running_mean = (1 - m) running_mean + m mean
  running_var  = (1 - m) running_var  + m var live / (live - 1);   num_batches_tracked += 1
  live < 2: var = 0, the three buffers untouched
backward from gy: gy' = gy mask [pre > 0]; g_beta = sum gy', g_gamma = sum gy' xhat;
  ga = gamma rstd (gy' - g_beta / live - xhat g_gamma / live); gx = rs ga, gres = ga; zeros past
  the live rows; the conv bias's gradient sum_v ga is identically 0.
mask: the project's hash dropout mask (oracle.regnn_oracle.dropout_mask) keyed on the sampler
state and the layer, the key of include/regnn_hip.h (regnn_nsm_step), divided by keep.

test_cpu_wide_bn.py holds this restatement to fp64 torch.nn.BatchNorm1d + relu under autograd."""
import numpy as np

from oracle import regnn_oracle as O

M64 = (1 << 64) - 1


def _mix(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def layer_seed(state, layer):
    """the dropout seed of `layer` for sampler state `state` (a list of ints)"""
    st = [int(v) for v in state]
    return _mix((st[0] & M64) ^ _mix(((st[1] << 40) ^ (st[3] << 8) ^ (layer + 0x51ED27)) & M64))


def keep16_of(p):
    return int(round((1.0 - float(p)) * 65536))


def drop_weight(state, layer, n, H, p):
    """mask / keep [n, H] (float64); p = 0: ones"""
    if not p > 0:
        return np.ones((n, H))
    k16 = keep16_of(p)
    return O.dropout_mask(layer_seed(state, layer), n, H, 4, k16).astype(np.float64) / (k16 / 65536)


def forward(x, gamma, beta, live, rs=None, bias=None, res=None, w=None, eps=1e-5, relu=True):
    """-> y [n, H] and the cache of backward(); w: drop_weight() or None"""
    x = np.asarray(x, np.float64)
    n, H = x.shape
    L = max(0, min(int(live), n))
    a = x[:L] * (1.0 if rs is None else np.asarray(rs, np.float64)[:L, None])
    if bias is not None:
        a = a + np.asarray(bias, np.float64)
    if res is not None:
        a = a + np.asarray(res, np.float64)[:L]
    mean = a.mean(0) if L else np.zeros(H)
    var = ((a - mean) ** 2).mean(0) if L >= 2 else np.zeros(H)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (a - mean) * rstd
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    pre = gamma * xhat + beta
    wl = np.ones((L, H)) if w is None else np.asarray(w, np.float64)[:L]
    y = np.zeros((n, H))
    y[:L] = (np.maximum(pre, 0.0) if relu else pre) * wl
    cache = dict(L=L, n=n, H=H, xhat=xhat, pre=pre, rstd=rstd, mean=mean, var=var, gamma=gamma,
                 w=wl, rs=rs, relu=relu)
    return y, cache


def backward(gy, c):
    """-> dict gx, gres, g_gamma, g_beta, g_bias"""
    L, n, H = c["L"], c["n"], c["H"]
    g = np.asarray(gy, np.float64)[:L] * c["w"]
    if c["relu"]:
        g = g * (c["pre"] > 0)
    g_beta, g_gamma = g.sum(0), (g * c["xhat"]).sum(0)
    ga = np.zeros((n, H))
    if L:
        ga[:L] = c["gamma"] * c["rstd"] * (g - g_beta / L - c["xhat"] * g_gamma / L)
    gx = ga if c["rs"] is None else ga * np.asarray(c["rs"], np.float64)[:, None]
    return dict(gx=gx, gres=ga, g_gamma=g_gamma, g_beta=g_beta, g_bias=np.zeros(H))


def buffers(c, running_mean, running_var, num_batches_tracked, momentum=0.1):
    """the three buffers after the forward of cache c"""
    rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    L = c["L"]
    if L < 2:
        return rm.copy(), rv.copy(), int(num_batches_tracked)
    return ((1 - momentum) * rm + momentum * c["mean"],
            (1 - momentum) * rv + momentum * c["var"] * L / (L - 1), int(num_batches_tracked) + 1)


def separate(x, gamma, beta, live, rs=None, bias=None, res=None, eps=1e-5, margin=1e-3):
    """x (fp32 array, changed in place) nudged so that no live pre-activation lies within `margin`
    of the relu's corner. An fp32 kernel and an fp64 reference may disagree on the sign of a
    pre-activation within a few 1e-6 of zero, which moves that element's gradient by the whole of
    gy: a property of the comparison, not of either side. Each pass moves the offending elements
    of a by 0.01 column standard deviations away from the corner (|gamma| >= 0.1 assumed: the
    pre-activation moves by >= margin) and recomputes the statistics."""
    assert np.abs(np.asarray(gamma)).min() >= 0.1
    for _ in range(8):
        _, c = forward(x, gamma, beta, live, rs, bias, res, None, eps)
        near = np.abs(c["pre"]) < margin
        if not near.any():
            return x
        sgn = np.where(c["pre"] >= 0, 1.0, -1.0) * np.sign(c["gamma"])
        step = 0.01 / c["rstd"] * sgn / (1.0 if rs is None else np.asarray(rs, np.float64)[:c["L"], None])
        x[:c["L"]][near] += step[near].astype(x.dtype)
    raise AssertionError("pre-activations still at the relu's corner")
