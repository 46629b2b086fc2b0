"""What the device-block GATv2 tests share (test_cpu_ns_gatv2.py, test_gpu_ns_gatv2.py): the
padded blocks are _ns_gat_blocks', the references _attention_ref's. A plain helper: no test lives
here, and nothing here needs a GPU.

* conv_restated  mag REGATv2Conv over a padded block as plain torch (any dtype), the attention by
                 _attention_ref.gatv2_reference with xs as score operand and message
* ladder_case    the ladder block's inputs of one (recipe, H, C): xs = fs (also the message),
                 xd = fd[:64], gy zero past the live rows
* ladder_ref     its fp64 reference and per-element scales in ops.ns_gatv2's terms, computed
                 once per case: g_xs = g_fs + g_ft (scale: the sum of the two), g_xd = g_fd
"""
import torch
import torch.nn.functional as F

import _attention_ref as R
import _ns_gat_blocks as B

FIXTURES = ["mag_regatv2conv_h4_res0", "mag_regatv2conv_h2_res1"]
RECIPES = ["unit", "wide"]
SHAPES = [(1, 64), (2, 32), (4, 16), (8, 64), (8, 8), (3, 8)]
# one shape per further column count per lane of the backward (regnn_ns_gatv2_bwd keeps 1, 2, 4, 8,
# 16 or 32 columns of a row in a lane; SHAPES reach 1 and 8): 2 with a ragged last pass (72 = 64
# + 8 columns, a head width that is no power of two), 4, 16, 32 at the widest row (2048) with 16
# heads and with the widest head (512). "unit" recipe only ("wide" needs a power-of-two C <= 64)
WIDTH_SHAPES = [(3, 24), (4, 64), (16, 64), (16, 128), (4, 512)]
KEYS = ("out", "g_xs", "g_xd", "g_att", "g_tab")

_CACHE = {}


def conv_restated(P, meta, blk, x, global_max=True):
    """mag.REGATv2Conv.forward((x, x[:cap_dst]), blk) restated in torch over the block's live
    entries (mag/regnn_layers.py:394-436): P = the conv's parameters by name, in x's dtype."""
    H, C = meta["heads"], meta["out_channels"]
    ptr, idx, rel = blk.live()
    xs = (x @ P["lin_src.weight"].t()).view(-1, H, C)
    xd = xs[:blk.n_dst]                                       # lin_dst is lin_src
    tab = F.leaky_relu(P["relation_weight"] * meta["scaling_factor"])
    out = R.gatv2_reference(ptr, idx, rel, xs, xd, P["att"], tab, xs, meta["negative_slope"],
                            global_max=global_max)
    out = out.reshape(-1, H * C) + P["bias"]
    if meta["residual"]:
        out = out + xd.reshape(-1, H * C)
    if meta["use_norm"] == "ln":
        out = F.layer_norm(out, (H * C,), P["norm.weight"], P["norm.bias"])
    return out


def ladder_block():
    if "blk" not in _CACHE:
        _CACHE["blk"] = B.ladder_block()
    return _CACHE["blk"]


def ladder_case(recipe, H, C):
    """(xs, xd, att, tab, gy, slope), fp32 CPU tensors"""
    c = B.LADDER
    fs, fd, att, tab, _ft, gy, slope = R.gatv2_inputs(recipe, c["cap_src"], H, C, c["n_rel"],
                                                      seed=200 + 7 * H + C)
    xd, gy = fd[:c["cap_dst"]].clone(), gy[:c["cap_dst"]].clone()
    gy[c["live_dst"]:] = 0.0                                  # no gradient into the padded rows
    return fs, xd, att, tab, gy, slope


def ladder_ref(recipe, H, C):
    """(want, scale): dicts over KEYS, fp64, left unchanged by the tests that share them"""
    key = (recipe, H, C)
    if key not in _CACHE:
        xs, xd, att, tab, gy, slope = ladder_case(recipe, H, C)
        ptr, idx, rel = ladder_block().live()
        w, s = R.gatv2_case_ref(ptr, idx, rel, xs, xd, att, tab, xs, gy, slope,
                                global_max="detached")
        want = {"out": w["out"], "g_xs": w["g_fs"] + w["g_ft"], "g_xd": w["g_fd"],
                "g_att": w["g_att"], "g_tab": w["g_tab"]}
        scale = {"out": s["out"], "g_xs": s["g_fs"] + s["g_ft"], "g_xd": s["g_fd"],
                 "g_att": s["g_att"], "g_tab": s["g_tab"]}
        _CACHE[key] = (want, scale)
    return _CACHE[key]
