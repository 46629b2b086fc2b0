"""Time and peak memory of the full-neighbour inference attention, fused against the chain of
existing operators, in one process:

    python tools/attn_infer_time.py [--scale 1] [--heads 8] [--hidden 64] [--reps 3] [--rounds 7]
                                    [--out FILE]

One graph -- mag_like(scale), 128-d inputs, REGNN 'regat' / 'regatv2' hidden 64 x 8 heads, 349
classes, 2 layers, LayerNorm, self-loop type 2 -- and for each kind one layer over every row
(regnn_hip.inference.RowBlock: all in-edges plus the self loops) in two forms:

  fused  ops.mag_attn_scores(form="fused") + finish: regnn_mag_attn_fwd (no [E, H] tensor),
         amax over [N, H], regnn_mag_attn_epilogue (softmax denominator, bias, LN, relu)
  chain  form="chain": regnn_gat_scores / regnn_gatv2_score_fwd -> amax over [E, H] ->
         regnn_edge_softmax_fwd(gmax, 1e-16) -> regnn_spmm_heads_fwd, then torch's bias /
         LayerNorm / relu

and the whole model.inference of 'regat' under either form. After a warm-up of both, `rounds`
timed windows of `reps` runs each, alternating the forms; a window is a host clock around the
runs ending in a device synchronise. Peak memory is torch.cuda.max_memory_allocated over one run
less what was allocated before it. Prints (and with --out writes) one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "re-gnn_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def windows(runs, reps, rounds):
    """{name: [ms per run, one per round]}: alternating windows"""
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                run()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / reps * 1e3)
    return ms


def peak_of(run):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def stats(v):
    return {"ms_median": round(statistics.median(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_infer_time: needs the GPU (no CPU timing)")
    import torch.nn.functional as F
    from regnn_hip import mag, ops, synth
    from regnn_hip.graph import RelGraph
    from regnn_hip.inference import ShardedInference
    dev = "cuda"
    gd = synth.mag_like(args.scale, seed=0, device=dev, zipf_s=1.1)
    keep = gd["rel"] <= 7
    rg = RelGraph(gd["src"][keep], gd["dst"][keep], gd["N"], dev)
    edge_type = gd["rel"][keep].to(torch.int64) - 1
    del keep, gd["src"], gd["dst"], gd["rel"]
    node_type = gd["ntype"]
    offs = torch.tensor([gd["type_offsets"][t] for t in synth.NTYPES], device=dev)
    local = torch.arange(gd["N"], device=dev) - offs[node_type]
    feats = synth.type_features(gd["counts"], {t: 128 for t in synth.NTYPES}, seed=1, device=dev)
    x_dict = {k: f for k, f in enumerate(feats)}

    def model(kind):
        torch.manual_seed(3)
        return mag.REGNN(128, args.hidden, 349, 2, 10.0, 0.0, {k: 128 for k in x_dict}, 7,
                         use_norm="ln", self_loop_type=2, model=kind,
                         heads=args.heads).to(dev).eval()

    H, C = args.heads, args.hidden
    out = {"workload": f"mag_like({args.scale:g}) full-neighbour inference, hidden {C} x {H} "
                       f"heads, 2 layers, LayerNorm", "N": int(gd["N"]), "reps_per_window": args.reps,
           "rounds": args.rounds}
    si = None
    for kind in ("regat", "regatv2"):
        m = model(kind)
        si = ShardedInference(m, rg, edge_type, node_type, local)
        out["entries"] = int(si.block.E)
        conv = m.convs[0]
        with torch.no_grad():
            _, xs = si.input(x_dict, 0)
            tab = F.leaky_relu(conv.relation_weight * conv.scaling_factor)
        kw = dict(att=conv.att) if conv.v2 else dict(att_src=conv.att_src, att_dst=conv.att_dst)
        ln = (conv.norm.weight, conv.norm.bias, conv.norm.eps)
        x3 = xs.view(-1, H, C)

        def layer(form):
            return ops.mag_attn_infer(si.block, x3, x3, "gatv2" if conv.v2 else "gat", tab,
                                      conv.negative_slope, bias=conv.bias, ln=ln, relu=True,
                                      form=form, **kw)

        runs = {"fused": lambda: layer("fused"), "chain": lambda: layer("chain")}
        a, b = runs["fused"](), runs["chain"]()
        diff = float((a - b).abs().max())
        del a, b
        peaks = {k: peak_of(r) for k, r in runs.items()}
        ms = windows(runs, args.reps, args.rounds)
        out[f"{kind}_layer"] = {k: {**stats(v), "peak_bytes": peaks[k]} for k, v in ms.items()}
        out[f"{kind}_layer"]["max_abs_diff"] = diff
        if kind == "regat":
            def whole(form):
                ops.MAG_ATTN_FORM["gat"] = form
                return si.run(x_dict, gather=None)

            default = ops.MAG_ATTN_FORM["gat"]
            runs = {"fused": lambda: whole("fused"), "chain": lambda: whole("chain")}
            for r in runs.values():
                r()
            peaks = {k: peak_of(r) for k, r in runs.items()}
            ms = windows(runs, 1, args.rounds)
            ops.MAG_ATTN_FORM["gat"] = default
            out["regat_inference"] = {k: {**stats(v), "peak_bytes": peaks[k]}
                                      for k, v in ms.items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
