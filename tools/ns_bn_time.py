"""Per-step time of NS 'regcn' training with use_norm 'bn' on the module engine, in one process:

    python tools/ns_bn_time.py [--scale 1] [--batch 512] [--hidden 512] [--steps 20] [--rounds 7]
                               [--out FILE]

One graph -- mag_like(scale), 128-d inputs, REGNN 'regcn' hidden 512, residual, 349 classes,
fan-out [25, 20], dropout 0.5, FlatAdam -- and three pipelined, captured trainers
(NSTrainer(engine="module"), run_steps) over it:

  A  use_norm 'bn' the way the module path ran it before ops.wide_bn_act: torch's addcmul / add /
     BatchNorm1d / relu / dropout over every row of the capacity-sized blocks. The same shape of
     work with WRONG statistics (the padded rows are counted); here only as the time to compare
     against. Built by switching mag.REGCNConv._bn_live off while A is constructed and captured.
  B  use_norm 'bn' as it runs now: ops.wide_bn_act (regnn_wide_bn_fwd / _bwd, three launches each
     way) over the live rows.
  C  the same model with use_norm 'ln' (ops.wide_ln_act, one launch each way), for context.

After warm-up runs of all three, `rounds` timed windows of `steps` steps each, alternating A, B,
C; a window is a host clock around the steps ending in a device synchronise. Prints (and with
--out writes) one JSON line: each leg's per-step median, min and max over the rounds (us).
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
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ns_bn_time: needs the GPU (no CPU timing)")
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

    def trainer(use_norm):
        torch.manual_seed(3)
        model = mag.REGNN(128, args.hidden, 349, 2, 10.0, args.dropout,
                          {k: 128 for k in x_dict}, 7, residual=True, use_norm=use_norm,
                          self_loop_type=2).to(dev)
        model.train()
        tr = NSTrainer(model, None, rg, [25, 20], args.batch,
                       torch.arange(n_paper, device=dev), x_dict, edge_type, node_type, local,
                       y, 7, seed=123, adam=dict(lr=1e-3), engine="module")
        assert tr.fused is None and tr._blocks_ok and tr.pipelined
        tr.capture(warmup=2)
        tr.run_steps(args.warmup)
        torch.cuda.synchronize()
        return tr

    live = mag.REGCNConv._bn_live
    mag.REGCNConv._bn_live = lambda self, blk: False      # leg A only: BatchNorm1d over all rows
    try:
        tr_a = trainer("bn")
    finally:
        mag.REGCNConv._bn_live = live
    trainers = {"bn_torch_all_rows": tr_a, "bn_live_rows": trainer("bn"), "ln": trainer("ln")}
    us = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_steps(args.steps)
            torch.cuda.synchronize()
            us[k].append((time.perf_counter() - t0) / args.steps * 1e6)
    out = {"workload": f"mag_like({args.scale:g}) NS step, regcn hidden {args.hidden}, residual, "
                       f"batch {args.batch}, fan-out [25, 20], dropout {args.dropout}, FlatAdam, "
                       "module engine, pipelined and captured",
           "steps_per_window": args.steps, "rounds": args.rounds}
    for k, v in us.items():
        out[k] = {"us_per_step_median": round(statistics.median(v), 1),
                  "min": round(min(v), 1), "max": round(max(v), 1),
                  "final_loss": float(trainers[k].loss)}
    a, b = out["bn_torch_all_rows"], out["bn_live_rows"]
    out["b_minus_a_us"] = round(b["us_per_step_median"] - a["us_per_step_median"], 1)
    out["a_spread_us"] = round(a["max"] - a["min"], 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
