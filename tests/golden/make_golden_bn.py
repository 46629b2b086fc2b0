"""Golden vectors of the NS model with batch norm: the REFERENCE's own REGNN class
(mag/regnn_ns.py:216-346) with use_norm 'bn' (BatchNorm1d after each conv over the layer's target
rows, mag/regnn_layers.py:64-65,134-135), self_loop_type 2, dropout 0, in TRAINING mode (batch
statistics, the running buffers updated), run in float64 on one sampled batch.

    python tests/golden/make_golden_bn.py     (writes tests/golden/nsbn_regnn_*.npz)

Like make_golden_residual.py this imports the reference at generation time only and no test runs
it; the helpers come from make_golden.py and the graph from make_golden_residual._schema_graph,
both of which stay as they are. The file names start with nsbn_, so no existing test's fixture
glob picks them up. Running it again rewrites the same bytes.

Both fixtures: the ogbn-mag-schema graph of make_golden_residual (354 nodes), K = 128, fan-out
[25, 20], a batch of 32 papers, 7 classes, the batch drawn by oracle.sampler_oracle.
  nsbn_regnn_h64_res1    hidden 64, residual convs
  nsbn_regnn_h128_res0   hidden 128, no residual
Each stores what make_golden_residual._store stores plus every BatchNorm buffer after the forward
as buf_<name> (running_mean, running_var, num_batches_tracked). Asserted before saving: every
layer's target count is >= 2 (BatchNorm needs two rows), and the outer block's targets are fewer
than its capacity 32 * 26 on the device sampler, so a capacity-sized block has padded rows which
the batch statistics must leave out.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_residual as MR  # noqa: E402

COUNTS = [170, 40, 14, 130]                        # author, field_of_study, institution, paper
SIZES, K, CLASSES = [25, 20], 128, 7


def gen(name, hidden, residual, graph_seed, model_seed):
    regnn_layers, SO = MR._setup()
    rng = np.random.default_rng(graph_seed)
    src, dst, edge_type, ntype, local, p0, batch = MR._schema_graph(rng, COUNTS)
    N = int(sum(COUNTS))
    ptr = MR._csr_ptr(dst, N)
    batch = (p0 + batch).astype(np.int64)
    seed, epoch, batch_idx = 77, 0, 2
    _, n_id, adjs = SO.neighbor_sample(ptr, src, batch.tolist(), SIZES, seed, epoch, batch_idx)
    live = [int(sz[1]) for _s, _d, _e, sz in adjs]            # outermost hop first
    assert all(v >= 2 for v in live), live
    assert live[-1] == batch.size
    cap_outer = batch.size * (SIZES[0] + 1)                   # the device sampler's hop-1 capacity
    assert live[0] < cap_outer, (live, cap_outer)
    y = np.full(N, -1, np.int64)
    y[p0:] = rng.integers(0, CLASSES, COUNTS[3])
    args = SimpleNamespace(model="regcn", feats_type=3, self_loop_type=2, no_re=False)
    REGNN = MG._reference_regnn_class(args, {t: COUNTS[t] for t in range(4)}, 3, regnn_layers)
    torch.manual_seed(model_seed)
    model = REGNN(K, hidden, CLASSES, 1, 2, 10.0, 0.0, {t: K for t in range(4)}, 7, residual,
                  False, use_norm="bn")
    MG._set_params(model, rng, ew_alpha=10.0)
    model.train()
    x_dict = {t: torch.from_numpy((MG.f32(rng, COUNTS[t], K) if t == 3 else
                                   rng.uniform(-0.5, 0.5, (COUNTS[t], K)).astype(np.float32))
                                  .astype(np.float64)) for t in range(4)}
    out, loss = MR._run(model, x_dict, n_id, adjs, edge_type, ntype, local, y[batch])
    st = dict(src=src, dst=dst, edge_type=edge_type, ntype=ntype, local=local, y=y, batch=batch,
              n_id=np.asarray(n_id, np.int64), logp=out, loss=loss.detach())
    MR._store(st, x_dict, adjs, model)
    bufs = dict(model.named_buffers())
    assert any(k.endswith("running_mean") for k in bufs)
    assert all(int(v) == 1 for k, v in bufs.items()
               if k.startswith("convs.") and k.endswith("num_batches_tracked"))
    MG._pack("buf_", bufs, st)
    MG.save(name,
            dict(model="mag.REGNN", feats_type=3, in_channels=K, hidden=hidden, classes=CLASSES,
                 num_layers=2, scaling_factor=10.0, num_edge_types=7, counts=COUNTS,
                 target_type=3, target_offset=p0, y_global=True, sizes=SIZES, seed=seed,
                 epoch=epoch, batch_idx=batch_idx, use_norm="bn", self_loop_type=2, dropout=0.0,
                 schema="ogbn-mag", residual=bool(residual), training=True, live=live,
                 capacity=[cap_outer, int(batch.size)], bn_eps=1e-5, bn_momentum=0.1), st)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    which = sys.argv[1:] or ["h64_res1", "h128_res0"]
    if "h64_res1" in which:
        gen("nsbn_regnn_h64_res1", 64, True, 277, 24)
    if "h128_res0" in which:
        gen("nsbn_regnn_h128_res0", 128, False, 278, 25)
