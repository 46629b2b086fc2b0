"""Golden vectors of REGATConv with head counts that are no power of two (H = 3, 6): the
REFERENCE's own layer/REGATConv.py in float64 on the dgl shim, exactly as make_golden.gen_layers
makes regatconv_h4_ee and its siblings.

    python tests/golden/make_golden_oddheads.py     (writes tests/golden/regatconv_h{3,6}_*.npz)

A generator of its own with its own seed: make_golden.py threads one rng through all of its
cases, so a case added there would change every fixture after it. Like make_golden.py this
imports the reference at generation time only and no test runs it; its helpers come from
make_golden.py, which stays as it is. Running it again rewrites the same bytes.

* regatconv_h3_ee:             in 32, H = 3, D = 8, relation table, no residual
* regatconv_h6_d8_ee_res_elu:  in 40, H = 6, D = 8, relation table, residual (res_fc), ELU

With a relation table these head counts take the generic (thread per (destination, head))
softmax kernels, whose backward bins the relation-table gradient per thread column.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

SEED = 4242


def main():
    MG._purge(["dgl", "layer", "model", "utils"])
    MG._use_paths([MG.SHIM, MG.REF])
    import dgl
    layer = importlib.import_module("layer")
    import torch.nn.functional as F

    rng = np.random.default_rng(SEED)
    gd = MG.make_hetero_graph(rng, [50, 65, 45, 30], 1700)
    g = dgl.DGLGraph((gd["src"], gd["dst"]), num_nodes=gd["N"])
    e_feat = torch.from_numpy(gd["rel"])
    N, R = gd["N"], gd["R"]
    alpha = 100.0
    cases = [
        ("h3_ee", 32, 8, 3, dict(residual=False, use_weight=True), None),
        ("h6_d8_ee_res_elu", 40, 8, 6, dict(residual=True, use_weight=True), "elu"),
    ]
    for tag, fin, fout, H, kw, act in cases:
        torch.manual_seed(SEED)
        m = layer.REGATConv(R, alpha, fin, fout, H, 0.0, 0.0, 0.01, kw["residual"],
                            F.elu if act else None, use_weight=kw["use_weight"])
        MG._set_params(m, rng, ew_alpha=alpha)
        feat = torch.from_numpy(MG.f32(rng, N, fin).astype(np.float64)).requires_grad_(True)
        out = m(g, feat, e_feat)
        gout = MG.f32(rng, *out.shape)
        out.backward(torch.from_numpy(gout.astype(np.float64)))
        st = {}
        MG._pack("g_", gd, st)
        st["feat"], st["gout"], st["out"] = feat.detach().numpy().astype(np.float32), gout, out
        st["grad_feat"] = feat.grad
        MG._pack("p_", MG._params(m), st)
        MG._pack("grad_", MG._grads(m), st)
        MG.save(f"regatconv_{tag}", dict(layer="REGATConv", alpha=alpha, in_feats=fin,
                                          out_feats=fout, num_heads=H, negative_slope=0.01,
                                          edge_feats=True, activation=act, **kw), st)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    main()
