"""Per-step time of the fused two-layer NS step with residual convs against without, in one
process (bench.py times the non-residual step only and has no residual switch):

    python tools/ns_residual_time.py [--scale 10] [--batch 512] [--steps 160] [--rounds 7]

bench.py's NS workload twice over one graph -- mag_like(scale), 128-d inputs, hidden 64, 349
classes, fan-out [25, 20], dropout 0.5, FlatAdam inside the step, pipelined and captured
(NSTrainer.capture / run_steps) -- once with residual=False and once with residual=True. After
warm-up runs of both, `rounds` timed windows of `steps` steps each, alternating the two trainers;
a window is a host clock around run_steps() ending in a device synchronise. Prints one JSON line
with each variant's per-step median, min and max over the rounds (us).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=10.0)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--dropout", type=float, default=0.5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ns_residual_time: needs the GPU (no CPU timing)")
    from regnn_hip import mag, synth
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import NSTrainer
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
    n_paper = gd["counts"]["paper"]
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    y = torch.full((gd["N"], 1), -1, dtype=torch.int64, device=dev)
    y[:n_paper, 0] = torch.randint(0, 349, (n_paper,), generator=gen, device=dev)

    def trainer(residual):
        torch.manual_seed(3)
        model = mag.REGNN(128, 64, 349, 2, 10.0, args.dropout, {k: 128 for k in x_dict}, 7,
                          residual=residual, use_norm="ln", self_loop_type=2).to(dev)
        tr = NSTrainer(model, None, rg, [25, 20], args.batch, torch.arange(n_paper, device=dev),
                       x_dict, edge_type, node_type, local, y, 7, seed=123, adam=dict(lr=1e-3),
                       engine="fused")
        assert tr.fused.two_layer and tr.fused.P.residual == int(residual) and tr.adam_fused
        tr.capture(warmup=2)
        return tr

    trs = {"plain": trainer(False), "residual": trainer(True)}
    for tr in trs.values():
        tr.run_steps(args.warmup)
    torch.cuda.synchronize()
    us = {k: [] for k in trs}
    for _ in range(args.rounds):
        for k, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_steps(args.steps)
            torch.cuda.synchronize()
            us[k].append((time.perf_counter() - t0) / args.steps * 1e6)
    out = {"workload": f"mag_like({args.scale:g}) NS step, batch {args.batch}, fan-out [25, 20], "
                       f"hidden 64, dropout {args.dropout}, fused Adam, captured",
           "steps_per_window": args.steps, "rounds": args.rounds,
           "launches": {k: tr.fused.launches() for k, tr in trs.items()}}
    for k, v in us.items():
        out[k] = {"us_per_step_median": round(statistics.median(v), 2),
                  "min": round(min(v), 2), "max": round(max(v), 2),
                  "final_loss": float(trs[k].loss)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
