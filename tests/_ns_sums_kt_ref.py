"""fp64 restatements for the sampler's sums launch at one input width per node type
(regnn_ns_hop_typed_sums_kt) and its layer-0 consumer (regnn_ns_slot_agg_kt / _bwd_kt), on plain
numpy arrays: tests/test_gpu_ns_type_layout.py::_oracle_sums restated with per-type widths over
oracle/sampler_oracle.py's draws, and the slot formulas of include/regnn_hip.h. Shared by
test_gpu_ns_sums_kt.py and test_cpu_ns_sums_kt.py; nothing here touches a GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import sampler_oracle as SO  # noqa: E402

WIDTH_SETS = [(256, 128, 128, 128), (128, 128, 128, 256), (64, 256, 128, 64),
              (256, 256, 256, 256), (64, 64, 64, 64)]
FANOUTS = [(3, 3), (3, 20), (3, 33)]           # 32 lanes one round / two rounds / 64 lanes + Floyd


def cols(widths):
    """type t's first column in a [sum K_t] row."""
    return np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)


def oracle_sums(g, csr, x64, widths, k0, k1, seed):
    """hop 0's n_id and, per row of the outer hop, the fp64 per-type sums [n1, sum K_t] (type t at
    column sum_{u<t} K_u), counts [n1, T], the self row [n1, max K_t] (zeros past its own width),
    the slot relations [n1, T + 1], the in-count and 1 / (in-count + 1), over the edges the
    sampler oracle draws. g: the graph's dict (ntype, local, etype, N, R); csr: (ptr, idx, eid)
    by target; x64: {type: [rows, K_t] float64}."""
    ptr, idx, eid = csr
    n_id, _, _, _ = SO.sample_hop(ptr, idx, list(range(g["N"])), k0, SO.hop_seed(seed, 0, 0, 0))
    hop_seed = SO.hop_seed(seed, 0, 0, 1)
    T, R, c = len(widths), g["R"], cols(widths)
    n1 = len(n_id)
    S, w = np.zeros((n1, int(c[-1]))), np.zeros((n1, T))
    xs, ur = np.zeros((n1, max(widths))), np.full((n1, T + 1), -1, dtype=np.int64)
    cnt = np.zeros(n1, dtype=np.int64)
    for i, t in enumerate(n_id):
        srcs, pos = SO.sample_row(ptr, idx, int(t), k1, hop_seed)
        cnt[i] = len(srcs)
        for u, p in zip(srcs, pos):
            tt = int(g["ntype"][u])
            S[i, c[tt]:c[tt + 1]] += x64[tt][int(g["local"][u])]
            w[i, tt] += 1
            r = int(g["etype"][eid[p]])
            assert ur[i, tt] in (-1, r)
            ur[i, tt] = r
        tt = int(g["ntype"][t])
        xs[i, :widths[tt]] = x64[tt][int(g["local"][t])]
        ur[i, T] = R + tt
    return n_id, dict(s_agg=S, s_w=w, u_self=xs, u_rel=ur, scnt=cnt, inv=1.0 / (cnt + 1.0))


def slot_fwd(U, cnt, xself, urel, tab, n_et, widths):
    """[S | w] of regnn_ns_slot_agg_kt in fp64: S [n, sum K_t], w [n, T]."""
    T, c = len(widths), cols(widths)
    n = U.shape[0]
    S, w = np.zeros((n, int(c[-1]))), np.zeros((n, T))
    for v in range(n):
        rs = int(urel[v, T])
        ts = rs - n_et if rs >= 0 else -1
        for t in range(T):
            r = int(urel[v, t])
            wr = tab[r] if r >= 0 else 0.0
            S[v, c[t]:c[t + 1]] = wr * U[v, c[t]:c[t + 1]]
            w[v, t] = wr * cnt[v, t]
            if t == ts:
                S[v, c[t]:c[t + 1]] += tab[rs] * xself[v, :widths[t]]
                w[v, t] += tab[rs]
    return S, w


def slot_bwd(U, cnt, xself, urel, gS, gw, n_et, widths, n_rel):
    """d tab [n_rel] of regnn_ns_slot_agg_bwd_kt in fp64."""
    T, c = len(widths), cols(widths)
    d = np.zeros(n_rel)
    for v in range(U.shape[0]):
        rs = int(urel[v, T])
        ts = rs - n_et if rs >= 0 else -1
        for t in range(T):
            r = int(urel[v, t])
            g = gS[v, c[t]:c[t + 1]]
            if r >= 0:
                d[r] += U[v, c[t]:c[t + 1]] @ g + cnt[v, t] * gw[v, t]
            if t == ts:
                d[rs] += xself[v, :widths[t]] @ g + gw[v, t]
    return d
