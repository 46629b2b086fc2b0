"""Output hashes of the typed layer-0 operators, for comparing two builds of the library bit by bit:

    REGNN_LIB=abx/libregnn_parent.so python tools/typed_bits.py
    python tools/typed_bits.py [--values FILE.npz]

Each run prints one JSON line {case: sha256 of the output's bytes}; two builds compute the same
bits where the lines are equal. Seeded inputs built here, on the block and table helpers of
tests/test_gpu_type_widths.py (the 24-row ladder block with rows of 0 .. 130 entries, extended to
8 node types for the <= 8-type kernels):

  agg/<widths>/<n_id|meta>/<plain|ext>/{S,w,d_rw}   ops.ns_typed_agg and its relation-weight
                                                    gradient, both hop forms, ext on and off
  lin/<widths>/O<O>[/groups]/{Y,gW<g>,gb<g>}        ops.typed_linear and every weight / bias
                                                    gradient; rows per type as in
                                                    test_typed_linear_mixed_widths (none, one forward
                                                    chunk and a row, a run across a wgrad chunk)

--values FILE.npz also keeps every agg case's d_rw vector, for the error of one build against
another (or against tests/test_gpu_type_widths.py's fp64 sums) where a hash differs.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "re-gnn_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

AGG_WIDTHS = [(64,) * 4, (128,) * 4, (128,) * 3, (64,) * 8, (128,) * 8, (256,) * 4,
              (256, 128, 128, 128), (64, 256, 128), (128, 64)]
# (widths, rows picked per type, weight group per type or None)
LIN_CASES = [((64,) * 4, (65, 129, 1025, 0), None), ((128,) * 4, (65, 129, 1025, 0), None),
             ((256,) * 4, (65, 129, 1025, 0), None), ((256, 128, 128, 128), (65, 129, 1025, 0), None),
             ((64, 256, 128), (0, 1025, 129), None),
             ((128,) * 4, (65, 129, 1025, 7), (0, 1, 1, 0)),
             ((256, 128, 128, 128), (65, 129, 1025, 7), (0, 1, 1, 2))]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _name(widths):
    return "x".join(map(str, widths))


def _run_agg(W, widths, meta, ext):
    """test_gpu_type_widths._run_agg for any width set (equal widths of 64 / 128 return S as
    [n_dst, T, K]): S, w and the relation-weight gradient under the test's gS / gw"""
    from regnn_hip import ops
    dev, T, SK = "cuda", len(widths), sum(widths)
    b = W._block(T)
    gS, gw = W._agg_case(widths)[:2]
    tables = [t.to(dev) for t in W._tables(widths)]
    assert ops.ns_typed_agg_ok(tables)
    rw = W._rw().to(dev).requires_grad_(True)
    tab = torch.nn.functional.leaky_relu(rw * 10.0)
    out = ops.ns_typed_agg(W._dev_block(b, meta), tab, torch.from_numpy(b["n_id"]).to(dev), tables,
                           torch.from_numpy(b["ntype"]).to(dev),
                           torch.from_numpy(b["local"]).to(dev), ext=ext)
    if ext:
        S, w = out[:, :SK], out[:, SK:SK + T]
    else:
        S, w = out[0].reshape(W.CAP_DST, SK), out[1]
    ((S * gS.to(dev)).sum() + (w * gw.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return S.detach(), w.detach(), rw.grad


def agg_cases(out, values):
    import test_gpu_type_widths as W
    W.COUNTS = W.COUNTS + [45, 40, 35, 30]          # four more node types for the 8-type blocks
    for widths in AGG_WIDTHS:
        for meta in (False, True):
            for ext in (False, True):
                S, w, g = _run_agg(W, widths, meta, ext)
                key = f"agg/{_name(widths)}/{'meta' if meta else 'n_id'}/{'ext' if ext else 'plain'}"
                out[key + "/S"], out[key + "/w"], out[key + "/d_rw"] = _sha(S), _sha(w), _sha(g)
                values[key + "/d_rw"] = g.cpu().numpy()


def lin_cases(out):
    from regnn_hip import ops
    dev = "cuda"
    for widths, picks, wgroup in LIN_CASES:
        for O in (64, 128):
            g = torch.Generator().manual_seed(sum(widths) + O + len(widths))
            T = len(widths)
            counts = [max(p, 1) + 40 for p in picks]
            ntype = torch.cat([torch.full((c,), t, dtype=torch.int64) for t, c in enumerate(counts)])
            local = torch.cat([torch.arange(c, dtype=torch.int64) for c in counts])
            offs = np.concatenate([[0], np.cumsum(counts)])
            ids = torch.cat([int(offs[t]) + torch.randperm(counts[t], generator=g)[:p]
                             for t, p in enumerate(picks)])
            n_id = ids[torch.randperm(ids.numel(), generator=g)].to(dev)
            tabs = [torch.randn(c, k, generator=g).to(dev) for c, k in zip(counts, widths)]
            wg = list(range(T)) if wgroup is None else list(wgroup)
            gk = {grp: widths[t] for t, grp in enumerate(wg)}
            Ws = [torch.randn(O, gk[i], generator=g).to(dev).requires_grad_(True)
                  for i in range(len(gk))]
            bs = [torch.randn(O, generator=g).to(dev).requires_grad_(True) for _ in gk]
            gy = torch.randn(n_id.numel(), O, generator=g).to(dev)
            assert ops.typed_linear_fusable(tabs, Ws, bs)
            y = ops.typed_linear(tabs, Ws, bs, ntype.to(dev), local.to(dev), n_id, wgroup=wgroup)
            y.backward(gy)
            torch.cuda.synchronize()
            key = f"lin/{_name(widths)}/O{O}" + ("/groups" if wgroup else "")
            out[key + "/Y"] = _sha(y)
            for i, (Wi, bi) in enumerate(zip(Ws, bs)):
                out[f"{key}/gW{i}"], out[f"{key}/gb{i}"] = _sha(Wi.grad), _sha(bi.grad)


def main():
    if not torch.cuda.is_available():
        sys.exit("typed_bits: needs the GPU")
    out, values = {}, {}
    agg_cases(out, values)
    lin_cases(out)
    print(json.dumps(out, sort_keys=True))
    if len(sys.argv) == 3 and sys.argv[1] == "--values":
        np.savez(sys.argv[2], **values)


if __name__ == "__main__":
    main()
