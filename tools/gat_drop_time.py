"""Time and peak memory of one REGATConv training step (forward + backward) with attention
dropout, fused against the three-operator path, in one process:

    python tools/gat_drop_time.py [--scale 1] [--heads 8] [--hidden 64] [--reps 3] [--rounds 7]
                                  [--limit 120] [--out FILE]

Two graphs -- mag_like(scale) with --zipf 0 (uniform) and with the default Zipf 1.1 (hub rows) --
and on each one layer.REGATConv (64 -> heads x hidden, relation bias, LeakyReLU 0.01) in train()
at p = 0.6 (16-bit draws) and p = 0.5 (8-bit draws), in three legs:

  A  ops.ATTN_DROP "torch": gat_attention -> nn.Dropout -> head_spmm (the [E, H] attention
     written, dropped by torch, gathered again; a, the dropped copy and torch's mask kept for
     the backward)
  B  "fused": ops.gat_fused(attn_drop=p) (regnn_gat_fused_fwd_drop, regnn_spmm_heads_bwd_drop)
  C  B's configuration with p = 0: the fused kernels without the mask, the floor

After a warm-up of every leg, `rounds` timed windows of `reps` steps each, alternating the legs; a
window is a host clock around the steps ending in a device synchronise. Peak memory is
torch.cuda.max_memory_allocated over one step less what was allocated before it. Every GPU step
(a graph build, a warm-up, a window, a peak run) runs under a watchdog of --limit seconds that
ends the process; an error ends the script. Prints (and with --out writes) one JSON line.
"""
import argparse
import faulthandler
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

LIMIT = [120]


def guarded(fn):
    """fn() under the watchdog: the process exits if it takes longer than the limit"""
    faulthandler.dump_traceback_later(LIMIT[0], exit=True)
    try:
        return fn()
    finally:
        faulthandler.cancel_dump_traceback_later()


def window(run, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


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
    ap.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gat_drop_time: needs the GPU (no CPU timing)")
    import dgl
    from layer import REGATConv
    from regnn_hip import ops, synth
    LIMIT[0] = args.limit
    dev = "cuda"
    H, C = args.heads, args.hidden
    out = {"workload": f"mag_like({args.scale:g}) REGATConv 64 -> {H} x {C}, relation bias, "
                       f"train(), forward + backward", "reps_per_window": args.reps,
           "rounds": args.rounds, "legs": {"A": "torch", "B": "fused", "C": "fused, p = 0"}}
    default = ops.ATTN_DROP["mode"]
    for zipf in (0.0, 1.1):
        def build():
            gd = synth.mag_like(args.scale, seed=0, device=dev, zipf_s=zipf)
            g = dgl.DGLGraph((gd["src"], gd["dst"]), num_nodes=gd["N"])
            rg = g.relgraph(dev)
            torch.cuda.synchronize()
            return gd, g, rg
        gd, g, rg = guarded(build)
        e_feat = gd["rel"].to(torch.int64)
        torch.manual_seed(3)
        conv = REGATConv(gd["R"], 100.0, 64, C, H, 0.0, 0.5, 0.01).to(dev).train()
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(gd["N"], 64, generator=gen, device=dev)
        gout = torch.randn(gd["N"], H, C, generator=gen, device=dev)
        params = list(conv.parameters())

        def step(mode, p):
            ops.ATTN_DROP["mode"] = mode
            conv.attn_drop.p = p
            y = conv(g, x, e_feat)
            y.backward(gout)
            for q in params:
                q.grad = None

        res = {"N": int(gd["N"]), "E": int(rg.E)}
        for p in (0.6, 0.5):
            runs = {"A": lambda: step("torch", p), "B": lambda: step("fused", p),
                    "C": lambda: step("fused", 0.0)}
            for r in runs.values():
                guarded(lambda: (r(), torch.cuda.synchronize()))
            peaks = {k: guarded(lambda: peak_of(r)) for k, r in runs.items()}
            ms = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, r in runs.items():
                    ms[k].append(guarded(lambda: window(r, args.reps)))
            res[f"p={p}"] = {k: {**stats(v), "peak_bytes": peaks[k]} for k, v in ms.items()}
        out[f"zipf={zipf:g}"] = res
        del conv, x, gout, g, rg, gd, e_feat
        torch.cuda.empty_cache()
    ops.ATTN_DROP["mode"] = default
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
