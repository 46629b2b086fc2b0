"""Device-resident neighbour-sampled (NS) step for the ogbn-mag path (mag/regnn_ns.py:206-214,
392-420) on MI355X: sampler, block aggregation, model step and optimizer with no host
synchronisation, so one training step is one HIP-graph replay.

* ``DeviceSampler`` — the per-hop sampler (regnn_ns_hop, include/regnn_hip.h) over buffers sized
  by capacity: batch B, then B*(k0+1), B*(k0+1)*(k1+1), ... targets / sources per hop. Counts live
  on the device (``sizes``); every later kernel reads them there.
* ``NSBlock`` — one hop's sampled block in the layout its aggregation reads (CSR by target,
  local ids, self loop last, uint8 relation ids, 1/in-count); RelGraph-compatible for ops.
* ``NSTrainer`` — one rank's data-parallel NS training step (regnn_ns_batch -> hops -> REGNN
  forward / nll / backward -> flat-bucket all-reduce -> Adam), captured in a HIP graph when
  asked. Rank r of W takes global batches r, r+W, ... of the epoch's shared permutation
  (SURVEY.md §8e); every rank runs the same number of steps per epoch.

The sampled indices follow the build's sampler spec (oracle/sampler_oracle.py, bit-exact).
"""
import contextlib
import ctypes
import gc
import os

import torch
import torch.nn.functional as F

from . import _lib as L
from .profile import enabled as profile_enabled, timed

M64 = (1 << 64) - 1


def _i64(u):
    """an unsigned 64-bit value as the int64 with the same bits."""
    u &= M64
    return u - (1 << 64) if u >= (1 << 63) else u


class NSBlock:
    """A sampled bipartite block (sources = n_id[:n_src], targets = n_id[:n_dst]).

    csr_ptr [n_dst+1] int32, csr_idx [E] local source ids (row v's self loop last), rel [E]
    uint8 0-based relation (edge type; num_edge_types + node type for the loop), pos [E] CSR
    position of the sampled edge in the global graph (-1: loop), row [E] each edge's target row,
    inv [n_dst] 1/(sampled + 1).
    n_dst / n_src / E are host ints: exact sizes (API path) or capacities (device engine)."""

    is_ns_block = True

    # True: every row ends with its self loop (self_loop_type 2, what DeviceSampler() writes);
    # False: sampled entries only, inv = 1 / max(sampled, 1) (DeviceSampler(self_loops=False):
    # self_loop_type 1 / 3)
    self_loops = True

    def __init__(self, ptr, idx, rel, pos, inv, n_dst, n_src, E, device, row=None):
        self.csr_ptr, self.csr_idx, self.rel, self.pos, self.inv = ptr, idx, rel, pos, inv
        self.row = row
        self.n_dst, self.n_src, self.E = int(n_dst), int(n_src), int(E)
        self.device = device

    def __iter__(self):                     # (edge_index, e_id, size) unpacking of the reference
        return iter((self, None, (self.n_src, self.n_dst)))

    def to(self, device):
        return self


class DeviceSampler:
    """Capacity-sized device sampler over a RelGraph (CSR by destination).

    etype: 0-based edge type per caller edge (mag edge_type), or None (relation 0);
    ntype: node type per global node (self-loop relation num_edge_types + ntype), or None.
    self_loops=False (mag self_loop_type 1 / 3): the hops append no self loop
    (regnn_ns_hop_noloop) -- a row holds its sampled entries only, inv = 1 / max(sampled, 1), the
    blocks carry ``self_loops = False``. CSR layout only: the strided layout, the transposed
    index, the edge meta and the input sums are refused (ValueError)."""

    def __init__(self, rg, sizes, batch_size, etype=None, ntype=None, num_edge_types=0,
                 share=None, self_loops=True):
        """share: another DeviceSampler over the same graph whose read-only tables (edge and
        node types) and dedup tables are reused (a second pipeline slot: the two never sample
        at the same time, and their dedup stamps never coincide)."""
        dev = rg.device
        self.rg, self.device = rg, dev
        self.self_loops = bool(self_loops)
        self.sizes_k = [int(k) for k in sizes]
        if not self.sizes_k or any(k < 1 or k > 64 for k in self.sizes_k):
            raise ValueError(f"device sampler fan-outs must lie in [1, 64], got {sizes}")
        if len(self.sizes_k) > 6:
            raise ValueError("at most 6 hops")
        self.B = int(batch_size)
        caps = [self.B]
        for k in self.sizes_k:
            caps.append(caps[-1] * (k + 1))
        if caps[-1] >= 2 ** 31:
            raise ValueError(f"sampler capacity {caps[-1]} exceeds int32")
        self.caps = caps
        self.num_edge_types = int(num_edge_types)
        n_nodes = max(rg.n_src, rg.n_dst)
        if share is not None:
            self.etype_csr, self.ntype = share.etype_csr, share.ntype
        elif etype is None:
            self.etype_csr = torch.zeros(rg.E, dtype=torch.uint8, device=dev)
        else:
            et = torch.as_tensor(etype).to(dev).reshape(-1)
            if et.numel() != rg.E:
                raise ValueError(f"etype has {et.numel()} entries, graph has {rg.E} edges")
            self.etype_csr = et[rg.csr_eid].to(torch.uint8).contiguous()
        if share is not None:
            pass
        elif ntype is None:
            self.ntype = torch.zeros(n_nodes, dtype=torch.int32, device=dev)
        else:
            self.ntype = torch.as_tensor(ntype).to(dev).to(torch.int32).contiguous()
        if int(self.num_edge_types) + (int(self.ntype.max().item()) if self.ntype.numel() else 0) > 255:
            raise ValueError("relation ids must fit uint8")
        self.state = torch.zeros(8, dtype=torch.int64, device=dev)
        self.sizes = torch.zeros(16, dtype=torch.int32, device=dev)
        self.n_id = torch.zeros(caps[-1], dtype=torch.int32, device=dev)
        if share is not None:
            # one stamp counter for both: the dedup tables need increasing stamps
            self.g2l, self.first = share.g2l, share.first
            if share.stamp_src is None:
                share.stamp_src = share.state[4:5].clone()
            self.stamp_src = share.stamp_src
        else:
            self.g2l = torch.zeros(n_nodes, dtype=torch.int64, device=dev)
            self.first = torch.full((n_nodes,), -1, dtype=torch.int64, device=dev)
            self.stamp_src = None
        self.hop_bufs, self.blocks = [], []
        for h, k in enumerate(self.sizes_k):
            cd = caps[h]
            ce = cd * (k + 1)
            nt = (ce + 1023) // 1024
            z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
            # tiles: the CSR de-duplication's nt tile counts and their ticket (nt + 1); status:
            # the strided de-duplication's look-back too (>= ceil(ce / 1024) tiles)
            self.hop_bufs.append(dict(samp=z(cd * k), spos=z(cd * k), scnt=z(cd), gsrc=z(ce),
                                      flag=z(ce, torch.uint8), tiles=z(nt + 1),
                                      status=z(max((cd + 1023) // 1024, nt), torch.int64)))
            blk = NSBlock(z(cd + 1), z(ce), z(ce, torch.uint8), z(ce),
                          torch.ones(cd, dtype=torch.float32, device=dev), cd, caps[h + 1], ce, dev,
                          row=z(ce))
            blk.state = self.state             # the batch's dropout key (the wide epilogue's)
            blk.self_loops = self.self_loops
            self.blocks.append(blk)
        self.local, self.edge_meta = None, [None] * len(self.sizes_k)
        self.meta_fresh = [False] * len(self.sizes_k)
        # sums_fresh[h]: the latest run_hops wrote hop h's layer-0 input sums (typed_sums path)
        self.sums_fresh = [False] * len(self.sizes_k)
        self.csc = [None] * len(self.sizes_k)      # per hop: (cnt, ptr, ent, long) or None
        # per hop: the CSR block's canonical transposed index (ops.NsTidx; the gather form of the
        # block attention backwards) or None; run_hops marks it stale, its build fresh
        self.tidx = [None] * len(self.sizes_k)
        # per hop with an index: each slot's rank in its source's segment (regnn_ns_hop csc_rank)
        self.csc_rank = [None] * len(self.sizes_k)
        # csc_defer[h]: a strided hop h leaves its index's scan + placement to the fused step's
        # head launch (FusedStep.defer_csc asks for it); csc_deferred[h]: the latest run_hops did
        self.csc_defer = [False] * len(self.sizes_k)
        self.csc_deferred = [False] * len(self.sizes_k)
        # csc_ride: a strided hop's counts + ranks ride the next hop's sums launch where one
        # follows (CSC_RIDE when the sampler is built; run_hops)
        self.csc_ride = CSC_RIDE["mode"] != "off"
        # strided: every hop's block in the fixed-stride layout (row i at i (k + 1), regnn_ns_hop
        # strided) -- the two-layer fused step's layout; False: the CSR layout the module path,
        # exact_adjs and the PyG-style API read
        self.strided = False
        # meta_only[h]: hop h writes only the edge meta its consumer reads (regnn_ns_hop
        # meta_only: no de-duplication, n_id not extended, sampled blk_idx unwritten)
        self.meta_only = [False] * len(self.sizes_k)
        # typed_sums[h]: hop h (meta-only, strided) also forms layer 0's input sums for the
        # fused step (regnn_ns_hop_typed_sums; FusedStep.enable_pre_sums), or None
        self.typed_sums = [None] * len(self.sizes_k)
        self.csc_sorted = None          # hop 0's index sorted per source (regnn_ns_csc_sort)
        self.hop_strided = [None] * len(self.sizes_k)   # per-hop layout override (run_hops)
        self._csc_jobs = {}
        self._csr_fresh = True

    def enable_edge_meta(self, local_node_idx, hop):
        """also write hop `hop`'s per-edge source node type and table row (regnn_ns_hop's
        optional outputs; what regnn_nsm_step's layer 0 gathers by)."""
        self._need_loops("enable_edge_meta (the edge meta feeds the fused step's layer 0)")
        self.local = torch.as_tensor(local_node_idx).to(self.device, torch.int64).contiguous()
        ce = self.blocks[hop].csr_idx.numel()
        self.edge_meta[hop] = (torch.zeros(ce, dtype=torch.int32, device=self.device),
                               torch.zeros(ce, dtype=torch.int64, device=self.device))
        self.meta_fresh[hop] = False          # written by the next run_hops
        return self.edge_meta[hop]

    def enable_csc(self, hop):
        """also build hop `hop`'s transposed index (regnn_ns_hop csc_*: per local source, its
        edges' target row << 8 | relation), what the fused step's transposed pass gathers by."""
        self._need_loops("enable_csc (the sampler-built transposed index)")
        ce = self.blocks[hop].csr_idx.numel()
        if ce > 32768:
            raise ValueError(f"the transposed index needs <= 32768 block edges, got {ce}")
        z = lambda n: torch.zeros(n, dtype=torch.int32, device=self.device)  # noqa: E731
        self.csc[hop] = (z(ce), z(ce + 1), z(ce), z(max(ce + 1, CSC_LONG_INTS)))
        self.csc_rank[hop] = z(ce)
        return self.csc[hop]

    def _need_loops(self, what):
        if not self.self_loops:
            raise ValueError(f"{what} is not built for a sampler with self_loops=False: "
                             "regnn_ns_hop_noloop writes the CSR layout only, without edge meta, "
                             "transposed index or input sums")

    def _check_noloop(self, strided):
        """a loop-less sampler's run_hops: every hop in the CSR layout, nothing beside the block"""
        if strided or any(bool(s) for s in self.hop_strided):
            self._need_loops("the fixed-stride layout (run_hops(strided=True) / hop_strided)")
        if any(self.meta_only) or any(m is not None for m in self.edge_meta):
            self._need_loops("enable_edge_meta / meta_only")
        if any(t is not None for t in self.typed_sums):
            self._need_loops("typed_sums (the sampler's layer-0 input sums)")
        if any(c is not None for c in self.csc):
            self._need_loops("enable_csc (the sampler-built transposed index)")

    def _csc_args(self, h):
        """regnn_ns_hop's csc_cnt .. csc_rank of hop h"""
        c = self.csc[h]
        return [L.ptr(t) for t in (*c, self.csc_rank[h])] if c is not None else [None] * 5

    # -- the per-step device work ------------------------------------------------------------
    def batch_from_perm(self, perm, rank=0, world=1):
        """regnn_ns_batch: this rank's next targets from the epoch permutation (device int64)."""
        L.call("regnn_ns_batch", L.ptr(perm), perm.numel(), self.B, int(rank), int(world),
               L.ptr(self.state), L.ptr(self.n_id), L.ptr(self.sizes),
               None if self.stamp_src is None else L.ptr(self.stamp_src), L.stream())

    def run_hops(self, meta_only=True, strided=None, before_sums=None):
        """every hop of the current batch; meta_only=False runs hops marked meta_only in full
        (a consumer that reads n_id / the local source ids, e.g. the module path); strided=False
        writes the CSR blocks whatever self.strided says (None: self.strided). before_sums:
        called right before the outer hop's sums launch (regnn_ns_hop_typed_sums), e.g. to make
        it wait on an event."""
        strided = self.strided if strided is None else bool(strided)
        if not self.self_loops:
            self._check_noloop(strided)
        # a hop's own layout (hop_strided[h] not None) wins over the call's: the module path
        # samples its outer hop strided with the input sums while hop 0 stays CSR
        hs = lambda h: strided if self.hop_strided[h] is None else self.hop_strided[h]  # noqa: E731
        rg = self.rg
        deferred, ride_place = -1, None
        for t in self.tidx:
            if t is not None:
                t.fresh = False                # older than the batch these hops sample
        for h, k in enumerate(self.sizes_k):
            b, blk = self.hop_bufs[h], self.blocks[h]
            sh = hs(h)
            if self._sums_path(h, sh, meta_only):
                if before_sums is not None:
                    before_sums()
                ts = self.typed_sums[h]
                # the graph's type layout (sampler_type_layout): the launch computes each slot's
                # type / table row / relation; and the per-slot meta only where something may
                # read it (ts["meta_unread"]: this hop's consumer reads the sums alone)
                lay = ts.get("layout")
                mode = SUMS_META["mode"]
                skip = (lay is not None and ts.get("meta_unread", False) and mode != "on" and
                        (mode == "off" or torch.cuda.is_current_stream_capturing()))
                rel, et, eo = (None, None, None) if skip else (blk.rel, *self.edge_meta[h])
                # one width per type (ts["widths"], a host int32 array): the _kt entry
                wd = ts.get("widths")
                with timed("ns_typed_sums"):
                    # the tables' storage type (ts["dtype"]: fp32 unless the x_dict is bf16)
                    L.call("regnn_ns_hop_typed_sums_dt" if wd is None else
                           "regnn_ns_hop_typed_sums_kt", L.ptr(rg.csr_ptr), L.ptr(rg.csr_idx),
                           L.ptr(self.etype_csr), L.ptr(self.ntype), self.num_edge_types, k, h,
                           L.ptr(self.state), L.ptr(self.sizes), L.ptr(self.n_id), self.caps[h],
                           L.ptr(b["scnt"]), L.ptr(rel), L.ptr(blk.inv), L.ptr(self.local),
                           L.ptr(et), L.ptr(eo), ts["tables"], ts.get("dtype", L.F32_CODE),
                           ts["T"], ts["K"] if wd is None else wd,
                           L.ptr(ts["s_agg"]), L.ptr(ts["s_w"]), L.ptr(ts["u_self"]),
                           L.ptr(ts["u_rel"]),
                           ctypes.addressof(self._csc_job(h - 1)) if deferred == h - 1 else None,
                           None if lay is None else ctypes.addressof(lay), L.stream())
                if ride_place is not None and ride_place[2]:
                    # the ranks rode this launch: hop h - 1's placement follows it on this stream
                    # (the index is complete when run_hops returns)
                    self._hop_call(ride_place[0], ride_place[1], meta_only, 5)
                deferred, ride_place = -1, None
                self.meta_fresh[h] = not skip
                self.sums_fresh[h] = True
                continue
            self.sums_fresh[h] = False
            # a strided hop with an index and no edge meta builds it in two halves, neither with a
            # wait between workgroups (regnn_ns_hop csc_rank: counts + ranks, then scan +
            # placement); later: the second half left to the fused step's head launch (strided = 4)
            has_index = bool(sh and self.csc[h] is not None and self.edge_meta[h] is None)
            later = has_index and bool(self.csc_defer[h])
            self.csc_deferred[h] = later
            # the first half in leading workgroups of the next hop's sums launch (CSC_RIDE;
            # regnn_ns_csc_job): this call stops after the de-duplication (strided = 2); the
            # placement follows the sums launch, or is the head launch's
            ride = (has_index and self.csc_ride and h + 1 < len(self.sizes_k) and
                    self._sums_path(h + 1, hs(h + 1), meta_only))
            self._hop_call(h, k, meta_only, 2 if ride else 4 if later else int(sh))
            deferred = h if ride else -1
            ride_place = (h, k, not later) if ride else None
            self.meta_fresh[h] = self.edge_meta[h] is not None
        if self.csc_sorted is not None and not self.csc_deferred[0]:
            # hop 0's transposed index in a canonical order (what the module path's gather reads:
            # NSTrainer._setup_module_slot), on the stream that built it
            _, cptr, cent, _ = self.csc[0]
            L.call("regnn_ns_csc_sort", L.ptr(self.sizes), 1, L.ptr(cptr), L.ptr(cent),
                   L.ptr(self.csc_sorted), cptr.numel() - 1, cent.numel(), L.stream())
        # the blocks now hold the CSR layout (readable by exact_adjs / model_blocks) or not
        self._csr_fresh = not strided

    def _sums_path(self, h, strided, meta_only):
        """hop h runs as regnn_ns_hop_typed_sums (the fused step's outer hop with layer 0's sums)"""
        return (self.typed_sums[h] is not None and strided and meta_only and self.meta_only[h]
                and self.edge_meta[h] is not None)

    def _csc_job(self, h):
        """regnn_ns_csc_job of hop h: its index's counts + ranks as a job of the next hop's sums
        launch (its buffers are fixed: built once)"""
        job = self._csc_jobs.get((h, True))    # keyed (hop, rank job) as before ABI 51
        if job is None:
            b, blk = self.hop_bufs[h], self.blocks[h]
            job = self._csc_jobs[(h, True)] = _NsCscJob(
                h, blk.csr_idx.numel(), L.ptr(b["gsrc"]), L.ptr(self.g2l), L.ptr(blk.csr_idx),
                L.ptr(self.csc[h][0]), L.ptr(self.csc_rank[h]))
        return job

    def _hop_call(self, h, k, meta_only, mode):
        """regnn_ns_hop of hop h with its buffers; mode: the call's `strided`"""
        rg, b, blk = self.rg, self.hop_bufs[h], self.blocks[h]
        if not self.self_loops:
            L.call("regnn_ns_hop_noloop", L.ptr(rg.csr_ptr), L.ptr(rg.csr_idx),
                   L.ptr(self.etype_csr), L.ptr(self.ntype), self.num_edge_types, k, h,
                   L.ptr(self.state), L.ptr(self.sizes), L.ptr(self.n_id), self.caps[h],
                   L.ptr(self.g2l), L.ptr(self.first), L.ptr(b["samp"]), L.ptr(b["spos"]),
                   L.ptr(b["scnt"]), L.ptr(b["gsrc"]), L.ptr(b["flag"]), L.ptr(b["tiles"]),
                   L.ptr(b["status"]), L.ptr(blk.csr_ptr), L.ptr(blk.csr_idx), L.ptr(blk.rel),
                   L.ptr(blk.pos), L.ptr(blk.row), L.ptr(blk.inv), L.stream())
            return
        L.call("regnn_ns_hop", L.ptr(rg.csr_ptr), L.ptr(rg.csr_idx), L.ptr(self.etype_csr),
               L.ptr(self.ntype), self.num_edge_types, k, h, L.ptr(self.state),
               L.ptr(self.sizes), L.ptr(self.n_id), self.caps[h], L.ptr(self.g2l),
               L.ptr(self.first), L.ptr(b["samp"]), L.ptr(b["spos"]), L.ptr(b["scnt"]),
               L.ptr(b["gsrc"]), L.ptr(b["flag"]), L.ptr(b["tiles"]), L.ptr(b["status"]),
               L.ptr(blk.csr_ptr), L.ptr(blk.csr_idx), L.ptr(blk.rel), L.ptr(blk.pos),
               L.ptr(blk.row), L.ptr(blk.inv),
               *((L.ptr(self.local), L.ptr(self.edge_meta[h][0]), L.ptr(self.edge_meta[h][1]))
                 if self.edge_meta[h] is not None else (None, None, None)),
               int(meta_only and self.meta_only[h] and self.edge_meta[h] is not None),
               *self._csc_args(h), mode, L.stream())

    def set_seed(self, base_seed, epoch, batch_idx):
        """host-driven batches (the PyG-style iterator): seed words + a fresh dedup stamp."""
        st = self.state.cpu()
        st[0], st[1], st[3] = _i64(int(base_seed)), int(epoch), int(batch_idx)
        if self.stamp_src is not None:
            self.stamp_src += 1
            st[4] = int(self.stamp_src.item())
        else:
            st[4] += 1
        self.state.copy_(st)

    def set_targets(self, targets):
        n = int(targets.numel())
        if n > self.B:
            raise ValueError(f"{n} targets exceed the sampler's batch capacity {self.B}")
        self.n_id[:n].copy_(targets.to(torch.int32))
        self.sizes[0:1].fill_(n)
        self.sizes[8:16].zero_()               # strided hops add their edge counts

    def _check_csr(self, what):
        if self.strided:
            raise RuntimeError(f"{what} reads CSR blocks, but this sampler writes the fused "
                               "step's fixed-stride layout (FusedStep set strided = True); call "
                               "run_hops(strided=False) first and read the blocks before the "
                               "next fused step")

    def model_blocks(self):
        """blocks in the model's layer order (outermost hop first, PyG adjs[::-1])."""
        if self.strided and not self._csr_fresh:
            self._check_csr("model_blocks()")
        return self.blocks[::-1]

    def exact_adjs(self):
        """PyG-style per-hop output at exact sizes (one host sync): [(edge_index [2, M] local
        (src, dst) without self loops, dst-major; e_id; (n_src, n_dst); NSBlock copy)], hop
        order (innermost first)."""
        if self.strided and not self._csr_fresh:
            self._check_csr("exact_adjs()")
        sz = self.sizes.cpu().tolist()
        out = []
        for h in range(len(self.sizes_k)):
            blk = self.blocks[h]
            n_dst, n_src, E = sz[h], sz[h + 1], sz[8 + h]
            ptr = blk.csr_ptr[:n_dst + 1].clone()
            idx, rel, pos = blk.csr_idx[:E].clone(), blk.rel[:E].clone(), blk.pos[:E].clone()
            inv = blk.inv[:n_dst].clone()
            cnt = (ptr[1:] - ptr[:-1]).to(torch.int64)
            dst_all = torch.repeat_interleave(torch.arange(n_dst, device=self.device), cnt)
            keep = pos >= 0
            src_l = idx[keep].to(torch.int64)
            dst_l = dst_all[keep]
            e_id = self.rg.csr_eid[pos[keep].to(torch.int64)]
            eb = NSBlock(ptr, idx, rel, pos, inv, n_dst, n_src, E, self.device)
            eb.self_loops = self.self_loops
            out.append((torch.stack([src_l, dst_l]), e_id, (n_src, n_dst), eb,
                        cnt - 1 if self.self_loops else cnt))
        return sz[len(self.sizes_k)], out


_P = ctypes.c_void_p
_MT, _ML = 8, 4


class _NsmParams(ctypes.Structure):
    """regnn_nsm_params (include/regnn_hip.h)."""
    _fields_ = [("n_types", ctypes.c_int32), ("k_in", ctypes.c_int32),
                ("n_layers", ctypes.c_int32), ("n_classes", ctypes.c_int32),
                ("alpha", ctypes.c_float), ("p_drop", ctypes.c_float),
                ("n_rel", ctypes.c_int32 * _ML),
                ("x_tab", _P * _MT), ("lin_w", _P * _MT), ("lin_b", _P * _MT),
                ("conv_w", _P * _ML), ("conv_b", _P * _ML), ("conv_rw", _P * _ML),
                ("ln_w", _P * _ML), ("ln_b", _P * _ML), ("out_w", _P), ("out_b", _P),
                ("g_lin_w", _P * _MT), ("g_lin_b", _P * _MT), ("g_conv_w", _P * _ML),
                ("g_conv_b", _P * _ML), ("g_conv_rw", _P * _ML), ("g_ln_w", _P * _ML),
                ("g_ln_b", _P * _ML), ("g_out_w", _P), ("g_out_b", _P), ("loss", _P),
                ("n_edge_types", ctypes.c_int32), ("rel_slots", ctypes.c_int32),
                ("two_layer", ctypes.c_int32), ("residual", ctypes.c_int32)]


class _NsmWork(ctypes.Structure):
    """regnn_nsm_work (include/regnn_hip.h)."""
    _fields_ = [("state", _P), ("sizes", _P), ("n_id", _P), ("cap", ctypes.c_int32 * (_ML + 1)),
                ("blk_ptr", _P * _ML), ("blk_idx", _P * _ML), ("blk_rel", _P * _ML),
                ("blk_inv", _P * _ML), ("ntype", _P), ("local", _P), ("labels", _P),
                ("wc", _P), ("gwc", _P), ("tabs", _P), ("xs", _P * _ML), ("gxs", _P * _ML),
                ("a", _P * _ML), ("stats", _P * _ML), ("ga", _P * _ML), ("edge_type", _P), ("edge_off", _P),
                ("s_agg", _P), ("s_w", _P), ("z", _P), ("beta", _P), ("nvalid", _P), ("slab", _P),
                ("u_self", _P), ("u_rel", _P), ("p0", _P), ("adam", _P), ("gh1", _P),
                ("csc_ptr0", _P), ("csc_ent0", _P), ("csc_long0", _P),
                ("stride", ctypes.c_int32 * _ML), ("blk_cnt", _P * _ML), ("part", ctypes.c_int32),
                ("hub_acc", _P), ("hub_ticket", _P), ("hub_terms", _P), ("split_finalize", ctypes.c_int32),
                ("pre_sums", ctypes.c_int32), ("csc_pending", ctypes.c_int32),
                ("csc_cap_e", ctypes.c_int32), ("csc_cnt0", _P), ("csc_rank0", _P)]

# include/regnn_hip.h REGNN_CSC_LONG_*: hub rows of a <= 32768-edge block, their <= 1024-entry
# pieces, and the csc_long buffer holding ids + piece table
_LONG_CAP = 32768 // 17 + 1
_CSC_PIECE = 1024                     # include/regnn_hip.h REGNN_CSC_PIECE (256: measured no faster,
#                                       the two-piece rows' ticket path cost what the split saved)
_MAX_PIECE = 32768 // _CSC_PIECE + _LONG_CAP
CSC_LONG_INTS = ((_LONG_CAP + 2) + 3) // 4 * 4 + 4 * _MAX_PIECE


class _NsCscJob(ctypes.Structure):
    """regnn_ns_csc_job (include/regnn_hip.h)."""
    _fields_ = [("hop", ctypes.c_int32), ("cap_e", ctypes.c_int32), ("gsrc", _P), ("g2l", _P),
                ("blk_idx", _P), ("csc_cnt", _P), ("csc_rank", _P)]


class _NsmAdam(ctypes.Structure):
    """regnn_nsm_adam (include/regnn_hip.h)."""
    _fields_ = [("param", _P), ("exp_avg", _P), ("exp_avg_sq", _P), ("grad_base", _P),
                ("n", ctypes.c_int64), ("lr", ctypes.c_float), ("beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("weight_decay", ctypes.c_float), ("grad_scale", ctypes.c_float),
                ("step", _P), ("ticket", _P)]


# regnn_nsm_step's two-layer form (re_nsm2.hip): L = 2 and at most 384 classes (its head's LDS)
TWO_LAYER_MAX_CLASSES = 384
# ... and a hop-0 block of at most this many entries (its transposed index)
TWO_LAYER_MAX_EDGES = 32768
_RESIDUAL_TWO_LAYER = ("residual convs run in the fused step's two-layer form only "
                       f"(2 layers, <= {TWO_LAYER_MAX_CLASSES} classes, hop-0 block capacity "
                       f"<= {TWO_LAYER_MAX_EDGES})")


def fused_unsupported(model, x_dict):
    """why regnn_nsm_step cannot run this model (None: it can). The fused step covers the
    reference configuration of mag/regnn_ns.py: model 'regcn', self_loop_type 2, use_norm 'ln',
    feats_type != 2, hidden 64, equal input widths 64 / 128, <= 8 node types, 2..4 layers,
    <= 448 classes; residual on every conv or on none, and residual in the two-layer form only
    (2 layers, <= TWO_LAYER_MAX_CLASSES classes; FusedStep also checks the hop-0 capacity).
    The input tables are contiguous and of one dtype: fp32, or bf16 at width 128 with <= 4 node
    types -- bf16 rows are read by the sampler's sums launch alone (regnn_ns_hop_typed_sums_dt),
    so FusedStep further needs its pre_sums conditions and raises where they do not hold."""
    if getattr(model, "model", None) != "regcn" or getattr(model, "feats_type", 3) == 2:
        return "model is not the feats_type-3 regcn"
    if model.self_loop_type != 2:
        return "self_loop_type != 2"
    convs = list(model.convs)
    if not 2 <= len(convs) <= _ML:
        return "2..4 layers"
    res = [bool(c.residual) for c in convs]
    if any(res) and not all(res):
        return "mixed residual flags across the convs"
    for c in convs:
        if c.use_norm != "ln" or tuple(c.weight.shape) != (64, 64):
            return "conv needs LayerNorm, hidden 64"
        if c.relation_weight.numel() > 64 or abs(c.scaling_factor - convs[0].scaling_factor) > 0:
            return "relation table > 64 or mixed scaling factors"
    keys = sorted(x_dict)
    if keys != list(range(len(keys))) or len(keys) > _MT:
        return "x_dict keys must be 0..T-1, T <= 8"
    dims = {int(x_dict[k].shape[1]) for k in keys}
    if len(dims) != 1 or dims.pop() not in (64, 128):
        return "input widths must be equal, 64 or 128"
    K = int(x_dict[keys[0]].shape[1])
    dts = {x_dict[k].dtype for k in keys}
    if len(dts) != 1:
        return "inputs must share one dtype (all fp32 or all bf16)"
    dt = dts.pop()
    if (dt not in (torch.float32, torch.bfloat16) or
            any(not x_dict[k].is_contiguous() for k in keys)):
        return "inputs must be contiguous fp32 (or bf16: width 128, <= 4 node types)"
    if dt == torch.bfloat16 and (K != 128 or len(keys) > 4):
        return "bf16 inputs need width 128 and <= 4 node types (the sampler's sums launch)"
    if len(keys) * (K + 1) > 600:              # regnn_nsm_step's composed-map bound
        return f"{len(keys)} node types x input width {K} exceed the fused step's tables"
    if model.out_lin.weight.shape[0] > 448 or model.out_lin.weight.shape[1] != 64:
        return "out_lin must be 64 -> <= 448"
    if res[0] and (len(convs) != 2 or model.out_lin.weight.shape[0] > TWO_LAYER_MAX_CLASSES):
        return _RESIDUAL_TWO_LAYER
    return None


def gat_blocks_unsupported(model, x_dict):
    """why NSTrainer(device_blocks=True) cannot train this model on the sampler's capacity-sized
    blocks (None: it can). Covered: mag.REGNN 'regat' (REGATConv over ops.ns_gat) with
    self_loop_type 2 (the self loops the sampler writes), use_norm 'ln' or none, fp32 tables
    (ops.BF16_ROWS "on": or all-bf16 ones, read by group_input's gather-fused Linear),
    1..16 heads and a head width that is a multiple of 4 in [4, 512]; and, with
    mag.GATV2_BLOCKS on, 'regatv2' (REGATv2Conv over ops.ns_gatv2) under the same conditions
    and heads x head width <= 2048. self_loop_type 1 / 3 with mag.NOLOOP_BLOCKS on (loop-less
    blocks, DeviceSampler(self_loops=False)): the same two attention models under the same
    conditions and 'regcn' (use_norm 'bn' too, over the live rows), all three on fp32 tables
    only; with that knob off (the default) types 1 / 3 are refused as before."""
    from . import mag, ops
    kind = getattr(model, "model", None)
    slt = getattr(model, "self_loop_type", None)
    noloop = slt in (1, 3) and mag.noloop_blocks_on()
    if noloop and any(torch.is_tensor(x) and x.dtype != torch.float32
                             for x in x_dict.values()):
        return (f"self_loop_type {slt}: loop-less blocks read fp32 input tables (bf16 tables are "
                "read through the sampler's input sums or ops.BF16_ROWS, neither built for them)")
    if kind == "regcn" and noloop:
        return None                            # (use_norm 'bn': NSTrainer checks ops.wide_bn_act)
    if kind == "regatv2" and mag.GATV2_BLOCKS["mode"] != "on":
        return ("regatv2: GATv2 scores have no device-block operator (ops.ns_gat covers "
                "REGATConv only); it stays on the exact-size path")
    if kind not in ("regat", "regatv2"):
        return f"model {kind!r} is neither 'regcn' nor 'regat'"
    op = "ops.ns_gat" if kind == "regat" else "ops.ns_gatv2"
    if slt != 2 and not noloop:
        return (f"self_loop_type {slt}: the sampler's blocks "
                "carry self_loop_type 2's self loops (relation num_edge_types + node type); "
                "REGNN_NOLOOP_BLOCKS=on (mag.NOLOOP_BLOCKS) samples loop-less blocks for "
                "types 1 / 3")
    for c in model.convs:
        if c.use_norm == "bn":
            return ("use_norm 'bn': batch statistics over the capacity-sized rows would include "
                    "the padded ones")
        if c.use_norm not in ("ln", "non", None):
            return f"use_norm {c.use_norm!r}"
        if not (1 <= c.heads <= 16 and c.out_channels % 4 == 0 and 4 <= c.out_channels <= 512):
            return (f"{c.heads} heads x {c.out_channels}: {op} takes 1..16 heads and a "
                    "head width that is a multiple of 4 in [4, 512]")
        if kind == "regatv2" and c.heads * c.out_channels > ops.NS_GATV2_MAX_WIDTH:
            return (f"{c.heads} heads x {c.out_channels}: ops.ns_gatv2 takes heads x head width "
                    f"<= {ops.NS_GATV2_MAX_WIDTH}")
    if any(torch.is_tensor(x) and x.dtype != torch.float32 for x in x_dict.values()):
        # ops.BF16_ROWS "on": group_input's gather-fused Linear reads all-bf16 tables
        # (NSTrainer._module_bf16_unsupported then checks their shapes)
        if not (ops.bf16_rows_on() and all(torch.is_tensor(x) and x.dtype == torch.bfloat16
                                           for x in x_dict.values())):
            return f"the attention path reads fp32 input tables (no bf16 tables for {kind!r})"
    return None


def _ops_bf16_rows_on():
    """ops.BF16_ROWS as a bool (ops is imported late throughout this module)"""
    from . import ops
    return ops.bf16_rows_on()


def fused_bf16_unsupported(model, sampler, x_dict):
    """why the fused step cannot read these bf16 input tables over this sampler's blocks (None: it
    can, or the tables are fp32). bf16 rows are read by the sampler's sums launch alone
    (regnn_ns_hop_typed_sums_dt; regnn_nsm_work.pre_sums): the step's own gathers (agg0) read
    fp32, so every condition of the input sums must hold. Changes nothing of the sampler."""
    keys = sorted(x_dict)
    if x_dict[keys[0]].dtype != torch.bfloat16:
        return None
    T, K = len(keys), int(x_dict[keys[0]].shape[1])
    two_layer = (len(model.convs) == 2 and
                 model.out_lin.weight.shape[0] <= TWO_LAYER_MAX_CLASSES and
                 sampler.blocks[0].csr_idx.numel() <= TWO_LAYER_MAX_EDGES)
    if PRE_SUMS["mode"] == "off":
        missing = "PRE_SUMS is off"
    elif not two_layer:
        missing = "not the two-layer step"
    elif K != 128 or T > 4:
        missing = "width 128 and <= 4 node types"
    elif STRIDED["mode"] == "off" or LEAN_LAST_HOP["mode"] == "off":
        missing = "the blocks are not strided (STRIDED / LEAN_LAST_HOP off)"
    elif max(sampler.sizes_k) > 63:
        missing = "a fan-out above 63"
    elif REL_SLOTS["mode"] == "off" or not relation_slots_ok(sampler, T):
        missing = "no relation slots (REL_SLOTS off, or a type pair with several relations)"
    else:
        return None
    return ("bf16 input tables are read by the sampler's sums launch only (pre_sums), which "
            f"does not apply: {missing}")


def fused_residual_unsupported(model, sampler):
    """why regnn_nsm_step cannot run this residual model over this sampler's blocks (None: it
    can, or the model has no residual convs): a hop-0 block past the two-layer form's transposed
    index would take the composed-map form, which has no residual."""
    if not any(bool(c.residual) for c in model.convs):
        return None
    if sampler.blocks[0].csr_idx.numel() > TWO_LAYER_MAX_EDGES:
        return _RESIDUAL_TWO_LAYER
    return None


# "auto": layer 0's relation-slot mode wherever the graph allows it; "off": the edge pass
# (rel0) always (tests compare the two)
REL_SLOTS = {"mode": "auto"}
# "on": the two-layer fused step's sampler writes its blocks in the fixed-stride layout (no
# row-offset scan, sampling and placement in one launch); "off": the CSR blocks (tests that
# inspect them, and the comparison of the two)
STRIDED = {"mode": "on"}
# "on": a one-rank FlatAdam trainer runs Adam inside the two-layer step's last launch; "off":
# the separate regnn_adam_flat launch (tests compare the two)
FUSED_ADAM = {"mode": "on"}
# "on": the pipelined trainer joins the sampler stream between the step's two parts (before
# layer 0's backward); "off": after the whole step (A/B)
SPLIT_JOIN = {"mode": os.environ.get("REGNN_NS_SPLIT_JOIN", "on")}
# "on": several ranks all-reduce the gradients the two-layer step has final after layer 1's
# transposed pass (early_grad_params, the bucket's head) while layer 0's backward runs on a
# forked stream, the rest after the step; "off" (default): one all-reduce of the whole bucket
# after the step. Measured on one rank with the several-rank structure (REGNN_NS_FORCE_EXCHANGE,
# mag-10x, hidden 64): 127.2 us split against 120.0 unsplit and 115.5 without an exchange -- the
# extra reduction launch and the fork / join cost more than the overlap hides while a
# collective's latency, not its bytes, sets its time
SPLIT_EXCHANGE = {"mode": os.environ.get("REGNN_NS_SPLIT_EXCHANGE", "off")}
# "on" (default): the module path (device blocks) samples the next batch on a second stream while
# the model trains on this one, as the fused step does; "off": in order. At hidden 512, mag-10x:
# round 3 (hipBLASLt GEMMs) 1.045 off / 1.09 on; round 4 (x6 GEMMs, interleaved pairs) 0.771 /
# 0.761 off against 0.757 / 0.756 on; round 5 (three interleaved 300-step pairs) 0.683-0.684
# off against 0.667-0.673 on
MODULE_PIPELINE = {"mode": os.environ.get("REGNN_NS_MODULE_PIPELINE", "on")}
# the module path's sampling lookahead (REGNN_NS_MODULE_AHEAD): 1 -- the next batch sampled beside
# each step, a fork and a join per step (each a marker on the model's queue: ~5 us of queue idle
# apiece in a kernel trace at hidden 512); G > 1 -- the fused engine's lookahead groups (2G slots,
# one fork and one join per group of up to G steps); 8 measured 412.3-412.5 against 416.7-416.8
# us per step for 4 at hidden 512, mag-10x (after this round's other module-path changes)
MODULE_AHEAD = {"n": int(os.environ.get("REGNN_NS_MODULE_AHEAD", "8"))}
# "on": the module path's out_lin + loss as ops.ns_lin_xent (labels, per-row loss and the mean in
# one launch; the loss backward with out_lin's bias gradient in one); "off": out_lin, ns_labels
# and ops.softmax_xent (A/B)
LIN_XENT = {"mode": os.environ.get("REGNN_NS_LIN_XENT", "on")}
# A strided hop's transposed index is built in two halves with no wait between workgroups
# (regnn_ns_hop csc_rank: counts + ranks, then every workgroup's own scan and placement); the two
# knobs below choose where the halves run. DESIGN section 4b has the measurements
# "on": the fused trainer's hop 0 runs the build's first half only and the step's head
# launch finishes the index on CUs it leaves idle (regnn_nsm_work csc_pending); "off": the
# placement on the sampler's queue; "auto" (default): "on" where hop 0's counts + ranks ride the
# sums launch (CSC_RIDE: the placement would otherwise be one more launch after the sums, and the
# sampler's chain per batch ends with the sums launch instead), else "off" (with the rank launch
# of its own the deferral measured within noise)
CSC_DEFER = {"mode": os.environ.get("REGNN_NS_CSC_DEFER", "auto")}
# "on" (default): where a strided hop's index build is followed by the sums launch (the fused
# trainer's hop 0), its counts + ranks run in leading workgroups of that launch instead of a
# launch of their own (regnn_ns_csc_job: a slot per thread, no wait), and the placement
# follows the sums launch (or rides the head launch, CSC_DEFER); "off": the rank launch of its
# own ahead of the sums. Every other hop sequence is the same either way
CSC_RIDE = {"mode": os.environ.get("REGNN_NS_CSC_RIDE", "on")}
# the head launch's dynamic-LDS limit (re_nsm2.hip): the deferred half's LDS must fit under it
_HEAD_LDS_MAX = 160 * 1024 - 2560
# the fused engine's sampling lookahead G: 2G sampler slots, each step samples the batch trained
# G steps later, and a G-step graph trains G slots while the sampler fills the other G on the
# second queue with one fork (the graph's root) and one join (its end) -- instead of a fork and
# a join per step, each a few us of queue idle on the model's chain. G = 1: two slots, the
# next batch sampled during this step and joined before layer 0's backward. Measured at
# mag-10x, hidden 64: 134.7 (G=1) / 129.1 (G=4) / 128.1 (G=8) us per step; 16 slots hold
# 0.9 GiB more HBM than 2.
# Round 5 (one rank, 300-step runs): G = 8 107.4-108.4, 16 106.5-108.3, 32 105.6-106.0 us (a
# fork / join per group). Default: 32 with one rank; 8 with several (every captured group holds
# one RCCL all-reduce per step, and that capture was only rehearsed at 8); REGNN_NS_AHEAD wins.
# Round 6: a timed run starts from an idle GPU (after a synchronisation), and a replay's nodes
# reach the queues only as fast as the host enqueues them, so the first group of a run sets how
# late the sampler's queue starts. With a 4-step lead group (PLAN_ORDER "lead4") the 20-step run
# the driver times measured (6 x 20 steps, medians): G = 32 desc 117.8, G = 32 lead4 114.2,
# G = 8 desc 114.0, G = 16 lead4 109.2-110.4 us per step; 160-step runs 106.0 / 105.4 (G = 32
# desc / lead4) against 106.4 (G = 16 lead4). Default: 16 with one rank (32 slots: half the
# lookahead memory of 32)
AHEAD = {"steps": int(os.environ["REGNN_NS_AHEAD"]) if "REGNN_NS_AHEAD" in os.environ else None}


def default_ahead(world):
    return AHEAD["steps"] if AHEAD["steps"] is not None else (16 if world == 1 else 8)
# "on": inside a lookahead group, the sampler's outer-hop sums launch for the group's batch i
# waits for the end of model step i - 1 (a model -> sampler edge only: the model never waits),
# placing it beside step i's agg0 / head; N: only every N-th batch (each edge costs a
# marker on the model's queue, ~4 us of idle before the next agg0; 6 x 20-step runs: on 111.0,
# 2 110.1, 4 110.2 us; 160 steps 106.2 / 105.5 / 105.5); "off": the sampler runs free
# "auto" (default): "on" where the fused trainer's strided hop 0 builds a transposed index (in
# two halves, deferred or not: the sampler's chain per batch reaches every step's edge in time,
# so each sums launch sits beside agg0 / head), else "2". DESIGN section 4b has the runs
SUMS_ALIGN = {"mode": os.environ.get("REGNN_NS_SUMS_ALIGN", "auto")}
# "on": the module path's outer hop forms layer 0's per-type input sums on the sampler's stream
# (relation slots; NSTrainer._module_pre_sums) and layer 0 reads them; "off": layer 0 gathers the
# sampled raw rows itself (regnn_ns_typed_agg, A/B)
MODULE_PRE_SUMS = {"mode": os.environ.get("REGNN_NS_MODULE_PRESUMS", "on")}
# "on": the module path samples hop 0 in the strided layout too (its last layer's forward reads
# the strided rows, its backward the transposed index); "off": hop 0 in the CSR layout (A/B)
MODULE_STRIDED = {"mode": os.environ.get("REGNN_NS_MODULE_STRIDED", "on")}
# "on": FlatAdam advances its step count with a one-element add and launches regnn_adam_flat
# without its end-of-grid ticket (ticket NULL); "off": the launch advances it behind the ticket
ADAM_PRE_STEP = {"mode": os.environ.get("REGNN_ADAM_PRE_STEP", "on")}
# "on": the module path's last hop runs meta-only when the model's layer 0 is the typed first
# layer (mag.REGNN.typed_first_layer_ok); "off": the full hop (A/B, tests)
MODULE_LEAN_HOP = {"mode": os.environ.get("REGNN_NS_MODULE_LEAN", "on")}
# "on": the fused step's last sampler hop runs meta-only (no dedup / n_id append); "off": the
# full hop (tests that inspect the outermost n_id / local ids)
LEAN_LAST_HOP = {"mode": "on"}
# "on": with relation slots (K = 128, T <= 4) the fused step's outer hop also forms layer 0's
# per-type input sums (regnn_ns_hop_typed_sums) on the sampler's stream, ahead of the model, and
# agg0 reads them (regnn_nsm_work.pre_sums); "off": agg0 gathers the raw rows itself (A/B, tests)
PRE_SUMS = {"mode": os.environ.get("REGNN_NS_PRE_SUMS", "on")}


# "on": where the graph's node ids are grouped by type (type_layout below), the sampler's sums
# launch computes each slot's source type, table row and relation from its node id instead of
# loading them from the per-edge / per-node tables (regnn_ns_type_layout); "off": the tables (A/B)
TYPE_LAYOUT = {"mode": os.environ.get("REGNN_NS_TYPE_LAYOUT", "on")}
# the sums launch's per-slot meta (blk_rel, edge_type, edge_off) once layer 0 reads the sums
# instead: "auto" (default): written by eager calls (a caller may inspect the block between
# steps), left out while a graph is captured (nothing in a replayed step reads them); "on" /
# "off": always / never written (never: only with the type layout)
SUMS_META = {"mode": os.environ.get("REGNN_NS_SUMS_META", "auto")}


def pair_relations(node_type, csr_ptr, csr_idx, etype_csr, T):
    """one pass over a graph's edges (CSR by target; plain tensors on any device): the [T, T]
    int64 table (target type, source type) -> the pair's edge relation, -1 where the graph has no
    such edge, and whether every pair has at most one relation (a pair with several keeps -1).
    Edges at a node whose type lies outside [0, T) are left out."""
    dev = csr_ptr.device
    ptr = csr_ptr.to(torch.int64)
    E = int(csr_idx.numel())
    present = torch.zeros(_MT * _MT * 256, dtype=torch.bool, device=dev)
    step = 1 << 26
    for a in range(0, E, step):
        b = min(E, a + step)
        pos = torch.arange(a, b, device=dev)
        dst = torch.searchsorted(ptr, pos, right=True) - 1
        st = node_type[csr_idx[a:b].to(torch.int64)].to(torch.int64)
        dt = node_type[dst].to(torch.int64)
        r = etype_csr[a:b].to(torch.int64)
        ok = (st >= 0) & (st < T) & (dt >= 0) & (dt < T)
        present[((dt * _MT + st) * 256 + r)[ok]] = True
    present = present.view(_MT, _MT, 256)[:T, :T]
    per_pair = present.sum(2)
    single = bool((per_pair <= 1).all().item())
    rel = torch.where(per_pair == 1, present.to(torch.float32).argmax(2),
                      torch.full_like(per_pair, -1))
    return rel.cpu(), single


def _pair_table(sampler, T):
    """pair_relations of the sampler's graph, cached on the graph."""
    rg = sampler.rg
    key = ("_regnn_rel_slots", sampler.num_edge_types, T)
    cache = getattr(rg, "_regnn_rel_slots", None)
    if cache is None or cache[0] != key:
        rel, ok = pair_relations(sampler.ntype, rg.csr_ptr, rg.csr_idx, sampler.etype_csr, T)
        cache = rg._regnn_rel_slots = (key, ok, rel)
    return cache


def relation_slots_ok(sampler, T):
    """regnn_nsm_params.rel_slots: True when every (target type, source type) pair of the graph
    has at most one edge relation (ogbn-mag's typed relations: each edge type joins one source
    type to one target type), so layer 0 may sum its input rows per source type unweighted.
    One pass over the graph's edges, cached on the graph."""
    return _pair_table(sampler, T)[1]


def type_layout(node_type, local_node_idx, csr_ptr, csr_idx, etype_csr, T, pairs=None):
    """The graph's type layout (regnn_ns_type_layout), or None when the graph has none: node ids
    grouped by type, as the reference's preprocessing leaves them (mag/regnn_ns.py:141-142).
    Plain tensors on any device. The layout holds when
      * node_type is non-decreasing with values in [0, T), T <= 4 (a type without nodes is fine:
        its offsets are equal and no id falls between them),
      * local_node_idx[u] == u - off[node_type[u]] for every node (off: the types' first ids),
      * every (target type, source type) pair of the edges has one relation (pairs: what
        pair_relations returned for this graph, else computed here).
    Returns dict(T, type_off = [0, .., nodes] (T + 1 ints), pair_rel = T x T lists, -1: none)."""
    if T < 1 or T > 4:
        return None
    nt = node_type.reshape(-1).to(torch.int64)
    lo = local_node_idx.reshape(-1).to(torch.int64)
    n = int(nt.numel())
    if n == 0 or lo.numel() != n or n >= 2 ** 31 - 1:
        return None
    if int(nt.min()) < 0 or int(nt.max()) >= T or bool((nt[1:] < nt[:-1]).any()):
        return None
    off = torch.zeros(T + 1, dtype=torch.int64, device=nt.device)
    off[1:] = torch.cumsum(torch.bincount(nt, minlength=T), 0)
    if not bool((lo == torch.arange(n, device=nt.device) - off[nt]).all()):
        return None
    rel, single = pairs if pairs is not None else pair_relations(nt, csr_ptr, csr_idx,
                                                                 etype_csr, T)
    if not single:
        return None
    return dict(T=T, type_off=[int(v) for v in off.cpu().tolist()],
                pair_rel=[[int(v) for v in row] for row in rel.tolist()])


class _NsTypeLayout(ctypes.Structure):
    """regnn_ns_type_layout (include/regnn_hip.h)."""
    _fields_ = [("n_types", ctypes.c_int32), ("type_off", ctypes.c_int64 * 5),
                ("pair_rel", (ctypes.c_int32 * 4) * 4)]


def layout_struct(lay):
    """type_layout's dict as the C struct."""
    s = _NsTypeLayout()
    s.n_types = lay["T"]
    for t, v in enumerate(lay["type_off"]):
        s.type_off[t] = v
    for a in range(4):
        for b in range(4):
            s.pair_rel[a][b] = lay["pair_rel"][a][b] if a < lay["T"] and b < lay["T"] else -1
    return s


def sampler_type_layout(sampler, T):
    """the sampler's graph's regnn_ns_type_layout struct (TYPE_LAYOUT on, the graph has the
    layout), else None; checked once per graph and cached on it as relation_slots_ok's verdict.
    Needs the sampler's table rows (enable_edge_meta)."""
    if TYPE_LAYOUT["mode"] == "off" or sampler.local is None:
        return None
    rg = sampler.rg
    key = ("_regnn_type_layout", sampler.num_edge_types, T, sampler.local.data_ptr())
    cache = getattr(rg, "_regnn_type_layout", None)
    if cache is None or cache[0] != key:
        _, ok, rel = _pair_table(sampler, T)
        lay = type_layout(sampler.ntype, sampler.local, rg.csr_ptr, rg.csr_idx,
                          sampler.etype_csr, T, pairs=(rel, ok))
        # (the checked tensor is kept: its address cannot pass to another while the verdict lives)
        cache = rg._regnn_type_layout = (key, None if lay is None else layout_struct(lay),
                                         sampler.local)
    return cache[1]


class FusedStep:
    """regnn_nsm_step over a DeviceSampler's blocks: the model's forward, nll loss and backward
    in eight launches (two layers), gradients written straight into each parameter's .grad (the
    caller's flat bucket views), loss into `loss`. Keeps every buffer it points the library at.
    A model with residual convs runs in the two-layer form only (P.residual); where that form
    does not apply (fused_residual_unsupported) the constructor raises ValueError."""

    def __init__(self, model, sampler, x_dict, node_type, local_node_idx, y_flat, loss):
        why = fused_unsupported(model, x_dict)
        if why is not None:
            raise ValueError(f"regnn_nsm_step does not cover this model: {why}")
        # (before anything of the sampler is changed and before any launch)
        why = fused_residual_unsupported(model, sampler)
        if why is not None:
            raise ValueError(f"regnn_nsm_step does not cover this model: {why}")
        dev = sampler.device
        self.device = dev
        nl = len(model.convs)
        if len(sampler.sizes_k) != nl:
            raise ValueError(f"{nl} layers need {nl} sampler hops, got {len(sampler.sizes_k)}")
        why = fused_bf16_unsupported(model, sampler, x_dict)
        if why is not None:
            raise ValueError(f"regnn_nsm_step does not cover these inputs: {why}")
        keys = sorted(x_dict)
        T, K = len(keys), int(x_dict[0].shape[1])
        C = int(model.out_lin.weight.shape[0])
        caps = sampler.caps
        self.keep = []                                 # every tensor the structs point at

        def ptr(t):
            self.keep.append(t)
            return t.data_ptr()

        def grad_ptr(p):
            if p.grad is None:                        # frozen parameter (no_re): scratch
                p_scratch = torch.zeros_like(p)
                return ptr(p_scratch)
            return ptr(p.grad)

        P = self.P = _NsmParams()
        P.n_types, P.k_in, P.n_layers, P.n_classes = T, K, nl, C
        P.alpha = float(model.convs[0].scaling_factor)
        P.p_drop = float(model.dropout) if model.training else 0.0
        for t, k in enumerate(keys):
            lin = model.lins[str(k)]
            P.x_tab[t] = ptr(x_dict[k])
            P.lin_w[t], P.lin_b[t] = ptr(lin.weight), ptr(lin.bias)
            P.g_lin_w[t], P.g_lin_b[t] = grad_ptr(lin.weight), grad_ptr(lin.bias)
        for l, c in enumerate(model.convs):
            P.n_rel[l] = c.relation_weight.numel()
            P.conv_w[l], P.conv_b[l], P.conv_rw[l] = ptr(c.weight), ptr(c.bias), ptr(c.relation_weight)
            P.ln_w[l], P.ln_b[l] = ptr(c.norm.weight), ptr(c.norm.bias)
            P.g_conv_w[l], P.g_conv_b[l] = grad_ptr(c.weight), grad_ptr(c.bias)
            P.g_conv_rw[l] = grad_ptr(c.relation_weight)
            P.g_ln_w[l], P.g_ln_b[l] = grad_ptr(c.norm.weight), grad_ptr(c.norm.bias)
        P.out_w, P.out_b = ptr(model.out_lin.weight), ptr(model.out_lin.bias)
        P.g_out_w, P.g_out_b = grad_ptr(model.out_lin.weight), grad_ptr(model.out_lin.bias)
        P.loss = ptr(loss)

        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        W = self.W = _NsmWork()
        W.state, W.sizes, W.n_id = ptr(sampler.state), ptr(sampler.sizes), ptr(sampler.n_id)
        for h, c in enumerate(caps):
            W.cap[h] = c
        for h, blk in enumerate(sampler.blocks):
            W.blk_ptr[h], W.blk_idx[h] = ptr(blk.csr_ptr), ptr(blk.csr_idx)
            W.blk_rel[h], W.blk_inv[h] = ptr(blk.rel), ptr(blk.inv)
        W.ntype = ptr(sampler.ntype)
        W.local = ptr(torch.as_tensor(local_node_idx).to(dev, torch.int64).contiguous())
        W.labels = ptr(y_flat.to(dev, torch.int64).contiguous())
        W.wc, W.gwc, W.tabs = ptr(z(T, K + 1, 64)), ptr(z(T, K + 1, 64)), ptr(z(nl, 64))
        for l in range(nl):
            n_src, n_dst = caps[nl - l], caps[nl - 1 - l]
            if l > 0:                                  # layer 0 reads the input tables directly
                W.xs[l], W.gxs[l] = ptr(z(n_src, 64)), ptr(z(n_src, 64))
            if l < nl - 1:
                W.a[l], W.stats[l] = ptr(z(n_dst, 64)), ptr(z(n_dst, 2))
            W.ga[l] = ptr(z(n_dst, 64))
        n0 = caps[nl - 1]
        et, eo = sampler.enable_edge_meta(local_node_idx, nl - 1)
        # layer 0 reads its block's sources by (type, table row) only: the last hop skips the
        # first-seen de-duplication and the local ids nothing here reads
        sampler.meta_only[nl - 1] = LEAN_LAST_HOP["mode"] != "off"
        W.edge_type, W.edge_off = ptr(et), ptr(eo)
        W.s_agg, W.z = ptr(z(n0, T, K)), ptr(z(n0, T, K))
        W.s_w, W.beta = ptr(z(n0, T)), ptr(z(n0, T))
        W.nvalid = ptr(z(1))
        # the two-layer step: layer 0 rows' fixed-point gradient sums and group_input's projection
        self.two_layer = (nl == 2 and C <= TWO_LAYER_MAX_CLASSES and
                          sampler.blocks[0].csr_idx.numel() <= TWO_LAYER_MAX_EDGES)
        # one decision for the library's slab size and step (regnn_nsm_params.two_layer): a
        # batch whose hop-0 block exceeds the transposed index runs the composed-map form
        P.two_layer = int(self.two_layer)
        P.residual = int(bool(model.convs[0].residual))
        if self.two_layer:
            W.p0 = ptr(z(caps[1], 64))
            W.gh1 = ptr(z(caps[0], 64))
            _, cptr, cent, clong = sampler.csc[0] or sampler.enable_csc(0)
            W.csc_ptr0, W.csc_ent0, W.csc_long0 = ptr(cptr), ptr(cent), ptr(clong)
            # exact hub-row sums of layer 1's transposed pass (kept zero between steps)
            W.hub_acc = ptr(torch.zeros(_MAX_PIECE * 64, dtype=torch.int64, device=dev))
            W.hub_ticket = ptr(torch.zeros(_LONG_CAP, dtype=torch.int32, device=dev))
            W.hub_terms = ptr(torch.zeros(3 * 64 + 1, dtype=torch.int64, device=dev))
            # the blocks in the fixed-stride layout: sampling and placement in one launch per hop
            sampler.strided = STRIDED["mode"] != "off"
            if sampler.strided:
                for h, k in enumerate(sampler.sizes_k):
                    W.stride[h] = k + 1
                    W.blk_cnt[h] = ptr(sampler.hop_bufs[h]["scnt"])
        self.adam = None
        P.n_edge_types = int(sampler.num_edge_types)
        P.rel_slots = int(REL_SLOTS["mode"] != "off" and relation_slots_ok(sampler, T))
        if P.rel_slots:
            W.u_self = ptr(z(n0, K))
            W.u_rel = ptr(torch.full((n0, T + 1), -1, dtype=torch.int32, device=dev))
        self.slab = z(_slab_floats(P, caps[0]))
        W.slab = ptr(self.slab)
        self.model, self.sampler, self.n_layers = model, sampler, nl
        # layer 0's parameter-free input sums on the sampler (it runs ahead of the model on its
        # own stream): the outer hop writes them straight into this step's s_agg / s_w / u_self
        # / u_rel and agg0 reads them instead of gathering the raw input rows
        if (PRE_SUMS["mode"] != "off" and self.two_layer and P.rel_slots and K == 128 and
                T <= 4 and sampler.strided and sampler.meta_only[nl - 1] and
                max(sampler.sizes_k) <= 63):
            self._tables = (ctypes.c_void_p * T)(*[x_dict[k].data_ptr() for k in keys])
            sampler.typed_sums[nl - 1] = dict(
                tables=self._tables, dtype=L.dtype_code(x_dict[keys[0]]), T=T, K=K, s_agg=self._buf(W.s_agg), s_w=self._buf(W.s_w),
                u_self=self._buf(W.u_self), u_rel=self._buf(W.u_rel),
                # agg0 and bwd0 then read s_agg / s_w / u_self / u_rel only: not the hop's meta
                layout=sampler_type_layout(sampler, T), meta_unread=True)
            W.pre_sums = 1
        elif x_dict[keys[0]].dtype != torch.float32:
            # (fused_bf16_unsupported names the same conditions: agg0 reads fp32 rows only)
            raise ValueError("regnn_nsm_step: bf16 input tables need the sampler's input sums "
                             "(pre_sums), which did not come on")

    def defer_csc(self):
        """hop 0's transposed index finished by this step's head launch instead of the sampler's
        queue (CSC_DEFER): the sampler's strided hop 0 then writes counts and ranks only
        (regnn_ns_hop strided = 4; with CSC_RIDE the outer hop's sums launch writes them and
        hop 0 stops after its de-duplication) and the step runs with csc_pending. Returns whether it
        applies: the two-layer step over strided blocks with hop 0's index and no edge meta, and
        the scan's LDS under the head launch's limit (else both launches stay on the sampler's
        queue)."""
        s, W = self.sampler, self.W
        ce = s.blocks[0].csr_idx.numel()
        mode = CSC_DEFER["mode"]
        if mode == "auto":                     # where hop 0's ranks ride the outer hop's sums launch
            mode = "on" if (s.csc_ride and len(s.sizes_k) > 1 and
                            s._sums_path(1, True, True)) else "off"
        ok = (self.two_layer and s.strided and s.csc[0] is not None and
              s.edge_meta[0] is None and mode != "off" and
              (ce + 64) * 4 <= _HEAD_LDS_MAX and
              # the index's grid row is no wider than the head's own (ceil(cap0 / 16) blocks of
              # 16 rows): only a fan-out of 64 exceeds it, and regnn_nsm_step refuses that
              -(-ce // 1024) <= -(-s.caps[0] // 16))
        s.csc_defer[0] = ok
        W.csc_pending, W.csc_cap_e = int(ok), ce
        if ok:
            W.csc_cnt0, W.csc_rank0 = s.csc[0][0].data_ptr(), s.csc_rank[0].data_ptr()
        return ok

    def _buf(self, addr):
        """the kept tensor whose data starts at addr."""
        return next(t for t in self.keep if torch.is_tensor(t) and t.data_ptr() == addr)

    def attach_adam(self, opt, grad_flat):
        """the optimizer step joins the last launch (two-layer step): Adam on each parameter
        element right after its gradient's reduction. opt: FlatAdam over the flat parameter
        bucket whose gradient bucket is grad_flat (every parameter's .grad a view into it)."""
        if not self.two_layer:
            raise ValueError("the fused optimizer needs the two-layer step")
        A = self.adam = _NsmAdam()
        A.param, A.exp_avg, A.exp_avg_sq = opt.p.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr()
        A.grad_base, A.n = grad_flat.data_ptr(), grad_flat.numel()
        A.lr, A.beta1, A.beta2, A.eps = opt.lr, float(opt.betas[0]), float(opt.betas[1]), opt.eps
        A.weight_decay, A.grad_scale = opt.weight_decay, opt.grad_scale
        A.step, A.ticket = opt.step_count.data_ptr(), opt.ticket.data_ptr()
        self.keep.extend([opt.p, opt.m, opt.v, grad_flat, opt.step_count, opt.ticket])
        self.W.adam = ctypes.addressof(A)

    def kernels(self):
        """the kernels one regnn_nsm_step launches, in order (bench.py's roofline label)."""
        if self.two_layer:
            ks = ["agg0", "head", "gather", "bwd0"] + ([] if self.P.rel_slots else ["rel0"])
            return ks + ["finalize+adam" if self.adam is not None else "finalize"]
        ks = ["prep", "agg0"] + ["agg"] * (self.n_layers - 2) + ["head"]
        ks += ["agg_bwd", "post_bwd"] * (self.n_layers - 1)
        ks += ["bwd0_rs" if self.P.rel_slots else "bwd0"]
        ks += [] if self.P.rel_slots else ["rel0"]
        return ks + ["finalize", "chain"]

    def launches(self):
        return len(self.kernels())

    def step(self, part=0):
        """part 0: the whole step; 1 / 2 (two-layer step): agg0 + head + gather / bwd0 +
        finalize, so the caller can order other work (the sampler's join) between them."""
        if part and not self.two_layer:
            raise ValueError("the step splits into parts only in its two-layer form")
        self.W.part = int(part)
        if part == 2:
            with torch.cuda.device(self.device):
                L.call("regnn_nsm_step", ctypes.addressof(self.P), ctypes.addressof(self.W),
                       torch.cuda.current_stream(self.device).cuda_stream)
            return
        # (with the sampler's sums the hop may leave the meta out: nothing of this step reads it)
        if not self.W.pre_sums and not self.sampler.meta_fresh[self.n_layers - 1]:
            raise RuntimeError("run the sampler's hops after building FusedStep: layer 0 reads the "
                               "per-edge source type / table row they write")
        if self.W.pre_sums and not self.sampler.sums_fresh[self.n_layers - 1]:
            # run_hops(meta_only=False) or run_hops(strided=False) samples the outer hop without
            # its input sums: agg0 / bwd0 would read an earlier batch's
            raise RuntimeError("the sampler's latest batch did not form layer 0's input sums "
                               "(run_hops with meta_only=True and the strided layout, as the "
                               "fused step's sampling does)")
        if self.two_layer and bool(self.W.csc_pending) != bool(self.sampler.csc_deferred[0]):
            # told pending, but the latest batch built its index in full (the head would rebuild
            # it from an earlier batch's ranks); or not told, and the gather would read an index
            # nobody finished
            raise RuntimeError("the step and the sampler's latest batch disagree about who "
                               "finishes hop 0's transposed index (FusedStep.defer_csc: step "
                               f"{bool(self.W.csc_pending)}, sampler "
                               f"{bool(self.sampler.csc_deferred[0])})")
        # train / eval decides the dropout (a captured graph keeps the value it was captured with)
        self.P.p_drop = float(self.model.dropout) if self.model.training else 0.0
        with torch.cuda.device(self.device), timed("nsm_step"):
            L.call("regnn_nsm_step", ctypes.addressof(self.P), ctypes.addressof(self.W),
                   torch.cuda.current_stream(self.device).cuda_stream)


def group_sizes(ahead):
    """the multi-step graph lengths at lookahead `ahead` > 1: ahead, ahead / 2, .., 2."""
    out, m = [], int(ahead)
    while m >= 2:
        out.append(m)
        m //= 2
    return out


# the order of a run's replays (plan_run): "desc" (the longest group first, as the greedy split
# finds them), "asc" (shortest first) or "leadL" (a group of L first, then the rest longest
# first). A replay's nodes reach the GPU queues while the host enqueues them; after an idle GPU
# (every timed run starts after a synchronisation) a short first group starts the sampler's
# queue early while the host enqueues the long groups behind it
PLAN_ORDER = {"mode": os.environ.get("REGNN_NS_PLAN", "lead4")}


def _split(k, ahead):
    """k steps as group lengths, longest first (group_sizes(ahead), ones for the rest)."""
    out = []
    while k > 0:
        m = next((m for m in group_sizes(ahead) if m <= k), 1)
        out.append(m)
        k -= m
    return out


def plan_sizes(k, ahead, order=None):
    """the group lengths plan_run replays for k steps, in order (PLAN_ORDER)."""
    order = order or PLAN_ORDER["mode"]
    sizes = _split(k, ahead)
    if order == "asc":
        return sorted(sizes)
    if order.startswith("lead"):
        lead = int(order[4:])
        if lead in group_sizes(ahead) and k > lead and sizes[0] > lead:
            return [lead] + _split(k - lead, ahead)
    return sizes


def plan_run(cur, k, ahead, n_slots, have=lambda m, start: True, order=None):
    """the replays NSTrainer.run_steps issues for k steps from slot `cur` at lookahead `ahead`
    > 1: [(m, start)], m = 1 for a one-step graph; the captured groups (`have`) of the greedy
    split of k into group lengths, in PLAN_ORDER's order, from wherever cur stands (a group
    without a captured graph runs as one-step graphs)."""
    out = []
    for m in plan_sizes(k, ahead, order):
        if m > 1 and not have(m, cur):
            for _ in range(m):
                out.append((1, cur))
                cur = (cur + 1) % n_slots
            continue
        out.append((m, cur))
        cur = (cur + m) % n_slots
    return out


def warm_walk(ahead, n_slots):
    """the replays capture() runs once each (a graph's first launch is slow), in training order
    from slot 0: for every group length m, n_slots times a group then one single step (the start
    advances by m + 1, odd, so it visits every slot) -- every (m, start) group and every
    one-step graph."""
    out, cur = [], 0
    for m in group_sizes(ahead):
        for _ in range(n_slots):
            out.append((m, cur))
            cur = (cur + m) % n_slots
            out.append((1, cur))
            cur = (cur + 1) % n_slots
    return out


@contextlib.contextmanager
def _capturing(g):
    """capture into g with the thread-local error mode: with several ranks the process group's
    watchdog thread polls the eager all-reduces' events meanwhile, which the global mode counts
    as an illegal call during capture (it invalidates the capture at random). Python's cyclic
    collector is held off until the capture has ended: torch.cuda.graph does not collect on
    entry, so a dead reference cycle from earlier (e.g. a trainer kept by a traceback, with its
    graphs and their pool memory) could otherwise be finalised in the middle of the capture,
    which aborts the process."""
    collecting = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            yield
    finally:
        if collecting:
            gc.enable()


def early_grad_params(model):
    """the parameters whose gradients the two-layer fused step has final after layer 1's
    transposed pass (regnn_nsm_work.split_finalize: reduced at the end of part 1): out_lin,
    layer 1 (weight, bias, relation table, LayerNorm) and layer 0's conv bias and LayerNorm."""
    c0, c1 = model.convs[0], model.convs[1]
    return [model.out_lin.weight, model.out_lin.bias, c1.weight, c1.bias, c1.relation_weight,
            c1.norm.weight, c1.norm.bias, c0.bias, c0.norm.weight, c0.norm.bias]


def _slab_floats(P, cap0):
    n = int(L._so.regnn_nsm_slab_floats(ctypes.addressof(P), int(cap0)))
    if n <= 0:
        raise RuntimeError("regnn_nsm_slab_floats rejected the parameters")
    return n


class FlatAdam:
    """torch.optim.Adam (mag/regnn_ns.py:495: lr, weight_decay) over one flat parameter bucket
    and its flat gradient bucket, one launch per step (regnn_adam_flat); the step count stays on
    the device, so the step can be captured in a HIP graph."""

    def __init__(self, params_flat, grads_flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0):
        self.p, self.g = params_flat, grads_flat
        self.m = torch.zeros_like(params_flat)
        self.v = torch.zeros_like(params_flat)
        dev = params_flat.device
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), betas, float(eps), \
            float(weight_decay)
        # the gradient's factor inside the launch (NSTrainer: 1 / ranks, the DP mean of the
        # SUM all-reduce, with no separate division pass)
        self.grad_scale = 1.0

    def step(self):
        pre = ADAM_PRE_STEP["mode"] != "off"
        if pre:
            # the step count advanced by a one-element add before the launch (capturable),
            # instead of the launch's end-of-grid ticket (regnn_adam_flat with ticket NULL)
            self.step_count.add_(1)
        L.call("regnn_adam_flat", L.ptr(self.p), L.ptr(self.g), L.ptr(self.m), L.ptr(self.v),
               self.p.numel(), self.lr, float(self.betas[0]), float(self.betas[1]), self.eps,
               self.weight_decay, self.grad_scale, L.ptr(self.step_count),
               None if pre else L.ptr(self.ticket), L.stream())


class NSTrainer:
    """One rank's NS training step (mag/regnn_ns.py:392-420) on the device sampler.

    model: mag.REGNN; opt: an optimizer over model.parameters() (Adam(capturable=True) for
    graph capture), or None for FlatAdam over a flat parameter bucket (`adam`: lr, betas, eps,
    weight_decay); train_idx: target nodes (the paper train split); y_global [N, 1] labels.
    The gradients live in one flat fp32 bucket (p.grad are views of it): one RCCL all-reduce
    per step for world > 1 (mag.flat_grad_allreduce's exchange), outside the captured graph.

    pipeline: 2 * ahead sampler slots (AHEAD; the module path: MODULE_AHEAD); while the model trains
    on one slot's batch, the batch `ahead` steps later is sampled into another on a second
    stream (the reference's NeighborSampler prefetches batches with DataLoader workers,
    mag/regnn_ns.py:206-208). Slot s deals global batches as rank + s * world of
    2 * ahead * world and the slots train round robin, so the batch sequence is the
    unpipelined one."""

    def __init__(self, model, opt, rg, sizes, batch_size, train_idx, x_dict, edge_type,
                 node_type, local_node_idx, y_global, num_edge_types, seed=0, rank=0, world=1,
                 shuffle=True, engine="auto", adam=None, pipeline=True, device_blocks=False):
        """device_blocks: also hand mag 'regat' models the capacity-sized device blocks
        (REGATConv over ops.ns_gat: no host sync, pipelined, capturable) instead of the
        exact-size adjs, and 'regatv2' models too where mag.GATV2_BLOCKS is on (REGATv2Conv
        over ops.ns_gatv2, the same step: CSR hops, lookahead 1, two slots, one-step graphs);
        raises ValueError where the blocks do not cover the model (gat_blocks_unsupported:
        'regatv2' with the knob off among them). 'regcn' / self_loop_type 2 is on the blocks
        either way. A model of self_loop_type 1 / 3 ('regcn', 'regat', 'regatv2' with its knob
        on) where mag.NOLOOP_BLOCKS is on: loop-less blocks (DeviceSampler(self_loops=False)) in
        the same step shape; the fused step and bf16 input tables are refused. With
        mag.NOLOOP_BLOCKS off (the default) such a model is refused here; without device_blocks
        it keeps the exact-size path."""
        self.model, self.opt = model, opt
        dev = rg.device
        self.device, self.rank, self.world = dev, int(rank), int(world)
        # self_loop_type 1 / 3 on device blocks: every slot samples without the appended loops
        # (opt-in: mag.NOLOOP_BLOCKS; off: such a model is refused below, as before)
        from . import mag as _mag
        self._noloop = (bool(device_blocks) and
                        getattr(model, "self_loop_type", None) in (1, 3) and
                        _mag.noloop_blocks_on())
        self.slots = [DeviceSampler(rg, sizes, batch_size, etype=edge_type, ntype=node_type,
                                    num_edge_types=num_edge_types,
                                    self_loops=not self._noloop)]
        self.cur, self._primed, self._trained = 0, False, 0
        self.train_idx = torch.as_tensor(train_idx).to(dev, torch.int64)
        self.perm = self.train_idx.clone()
        self.shuffle, self.seed = shuffle, int(seed)
        self.x_dict, self.node_type, self.local_node_idx = x_dict, node_type, local_node_idx
        self.edge_type = torch.as_tensor(edge_type).to(dev, torch.int64)
        self.y_flat = y_global.reshape(-1).to(dev, torch.int64)
        # the module path hands 'regcn' / self_loop_type 2 the capacity-sized device blocks (no
        # host sync: capturable); every other REGNN conv (regat unless device_blocks, regatv2,
        # other self-loop types) gets the PyG-style exact-size adjs and edge types (one host sync
        # per step)
        self._blocks_ok = (getattr(model, "model", None) == "regcn" and
                           getattr(model, "self_loop_type", None) == 2)
        # device_blocks: 'regat' too (mag.REGATConv reads the CSR blocks through ops.ns_gat), and
        # 'regatv2' with mag.GATV2_BLOCKS on (mag.REGATv2Conv through ops.ns_gatv2);
        # refused with a reason where the blocks do not apply (never a silent fall-back)
        self._gat_blocks = self._gat_src_gather = False
        if device_blocks and not self._blocks_ok:
            why_not = gat_blocks_unsupported(model, x_dict)
            if why_not is not None:
                raise ValueError(f"device_blocks=True does not cover this model: {why_not}")
            if engine == "fused":
                raise ValueError(
                    "device_blocks=True: "
                    + (f"a self_loop_type {model.self_loop_type} model" if self._noloop
                       else "'regat'")
                    + " runs on the module path, not the fused step"
                    + (" (regnn_nsm_step aggregates self_loop_type 2's blocks only)"
                       if self._noloop else ""))
            # (a loop-less 'regcn' takes the attention models' step shape: every hop CSR,
            # lookahead 1, two slots, one-step graphs)
            self._blocks_ok = self._gat_blocks = True
            # ops.NS_GAT_SRC "gather": every slot owns its hops' transposed-index buffers and
            # builds them beside the hops (_sample); the backwards then use no float atomics
            from . import ops as _ops
            self._gat_src_gather = (_ops.ns_gat_src_mode() == "gather" and
                                    getattr(model, "model", None) != "regcn")
        # use_norm 'bn' on the capacity-sized blocks: the batch statistics are taken over the
        # block's live rows by ops.wide_bn_act, never by torch's BatchNorm1d over the padded rows;
        # where that operator does not cover a conv the trainer refuses (no silent fall-back)
        if self._blocks_ok and getattr(model, "model", None) == "regcn":
            from . import ops as _ops
            for i, c in enumerate(getattr(model, "convs", [])):
                if getattr(c, "use_norm", None) != "bn":
                    continue
                bad = _ops.wide_bn_module_why_not(c.norm, int(c.out_channels), c.bias)
                if bad is not None:
                    raise ValueError(
                        f"use_norm 'bn': conv {i} cannot take its batch statistics over the "
                        f"block's live rows (ops.wide_bn_act): {bad}; torch's BatchNorm1d would "
                        "include the capacity-sized block's padded rows")
        self.params = [p for p in model.parameters() if p.requires_grad]
        # every parameter starts on a 16-byte boundary of the flat buckets (the fused step's
        # finalize sums and steps 4 aligned elements per thread); the pad elements stay zero.
        # Two-layer fused step: the gradients final after layer 1's transposed pass lead the
        # bucket ([0, n_early)), so several ranks all-reduce them while layer 0's backward runs.
        why = fused_unsupported(model, x_dict)
        if why is None:
            # a residual model whose hop-0 block exceeds the two-layer form: "auto" takes the
            # module path for every slot, "fused" gets FusedStep's error (below)
            why = fused_residual_unsupported(model, self.slots[0])
        # bf16 input tables (all of them, or none): read by the sampler's sums launch alone
        self._bf16 = any(torch.is_tensor(x) and x.dtype == torch.bfloat16
                         for x in x_dict.values())
        if why is None and self._bf16:
            why = fused_bf16_unsupported(model, self.slots[0], x_dict)
        if self._bf16 and (engine == "module" or why is not None):
            # (before any buffer is built) the module path reads bf16 tables only through the
            # sampler's input sums (_module_pre_sums)
            bad = self._module_bf16_unsupported(self.slots[0])
            if bad is not None and engine != "fused":
                raise ValueError(f"bf16 input tables: {bad}")
        early = []
        if engine != "module" and why is None and len(model.convs) == 2:
            ids = {id(p) for p in self.params}
            early = [p for p in early_grad_params(model) if id(p) in ids]
        eids = {id(p) for p in early}
        order = early + [p for p in self.params if id(p) not in eids]
        offs, o = {}, 0
        for p in order:
            offs[id(p)] = o
            o += (p.numel() + 3) // 4 * 4
            if p is (early[-1] if early else None):
                self.n_early = o
        if not early:
            self.n_early = 0
        self.offsets = [offs[id(p)] for p in self.params]
        self.flat = torch.zeros(o, dtype=torch.float32, device=dev)
        for p, o in zip(self.params, self.offsets):
            p.grad = self.flat[o:o + p.numel()].view_as(p)
        if opt is None:
            # the parameters become views of one flat bucket too, and one launch updates them
            # all (FlatAdam; `adam` = torch.optim.Adam's keyword arguments)
            self.pflat = torch.zeros_like(self.flat)
            for p, o in zip(self.params, self.offsets):
                self.pflat[o:o + p.numel()].copy_(p.detach().reshape(-1))
                p.data = self.pflat[o:o + p.numel()].view_as(p)
            self.opt = opt = FlatAdam(self.pflat, self.flat, **(adam or {}))
            # the data-parallel mean of the SUM all-reduce, inside Adam's launch: no division
            # pass between the exchange and the update (p.grad holds the rank sum)
            opt.grad_scale = 1.0 / self.world
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        # the module path's backward seed d loss / d loss = 1 (autograd would fill one per step)
        self._loss_seed = torch.ones((), dtype=torch.float32, device=dev)
        # ops.ns_lin_xent's last-workgroup ticket (zero between launches)
        self._xent_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        # engine: "fused" = regnn_nsm_step (the model's forward / loss / backward in eight HIP
        # launches), "module" = the mag.REGNN autograd path, "auto" = fused where it applies
        if engine == "fused" and why is not None:
            raise ValueError(f"fused NS step unavailable: {why}")
        self.fused = None
        if engine != "module" and why is None:
            self.fused = FusedStep(model, self.slots[0], x_dict, node_type, local_node_idx,
                                   self.y_flat, self.loss)
        # the module path on device blocks (regcn, self-loop type 2): capturable, and pipelined
        # like the fused step (the next batch sampled on a second stream)
        self._module_lean = (self.fused is None and self._blocks_ok and
                             MODULE_LEAN_HOP["mode"] != "off" and
                             getattr(model, "typed_first_layer_ok", lambda _x: False)(x_dict))
        if self.fused is None and self._blocks_ok:
            self._setup_module_slot(self.slots[0])
        # (ops.BF16_ROWS "on": without the input sums layer 0 reads the bf16 rows itself)
        if self._bf16 and self.fused is None and not _ops_bf16_rows_on() and \
                getattr(self.slots[0].blocks[-1], "pre_sums", None) is None:
            raise ValueError("bf16 input tables: the module path's input sums (_module_pre_sums) "
                             "did not come on")
        # REGNN_NS_PIPELINE=0: no second stream (a profiling aid: every kernel's time alone)
        pipeline = pipeline and os.environ.get("REGNN_NS_PIPELINE", "1") != "0"
        self.pipelined = bool(pipeline) and (self.fused is not None or
                                             (self._blocks_ok and MODULE_PIPELINE["mode"] != "off"))
        # the sampling lookahead (fused engine: default_ahead; the module path: MODULE_AHEAD)
        self.ahead = 1
        if self.pipelined:
            # 'regat' / 'regatv2' on device blocks: lookahead 1 whatever MODULE_AHEAD says (two
            # slots, one-step graphs only: every captured graph keeps a private pool of activations,
            # 573 MB per [cap_src, 512] tensor at 8 heads x 64, batch 512, fan-out [25, 20])
            self.ahead = max(1, int(default_ahead(self.world) if self.fused is not None
                                    else 1 if self._gat_blocks else MODULE_AHEAD["n"]))
        if self.pipelined:
            for j in range(1, 2 * self.ahead):
                self.slots.append(DeviceSampler(
                    rg, sizes, batch_size, num_edge_types=num_edge_types, share=self.slots[0],
                    self_loops=not self._noloop))
            if self.fused is not None:
                self.fused_slots = [self.fused] + [
                    FusedStep(model, s, x_dict, node_type, local_node_idx, self.y_flat, self.loss)
                    for s in self.slots[1:]]
            else:
                for s in self.slots[1:]:
                    self._setup_module_slot(s)
            # the sampler's stream; REGNN_NS_SIDE_PRIORITY (-1: high) for A/B runs
            self._side = torch.cuda.Stream(device=dev,
                                           priority=int(os.environ.get("REGNN_NS_SIDE_PRIORITY", "0")))
        # one rank, FlatAdam, two-layer step: the optimizer runs inside the step's last launch
        # (no all-reduce sits between the backward and the update)
        self.adam_fused = (self.fused is not None and self.fused.two_layer and self.world == 1
                           and isinstance(self.opt, FlatAdam) and FUSED_ADAM["mode"] != "off")
        if self.adam_fused:
            for fs in (self.fused_slots if self.pipelined else [self.fused]):
                fs.attach_adam(self.opt, self.flat)
        # the fused engine only, where CSC_DEFER asks for it (by default where hop 0's ranks ride
        # the sums launch): each slot's head
        # launch finishes the transposed index its sampler left at counts + ranks
        if self.fused is not None:
            for fs in (self.fused_slots if self.pipelined else [self.fused]):
                fs.defer_csc()
        self.graphs = None
        self.exchange_in_graph = False         # capture() sets it: the all-reduce is in the graphs
        # tests: all-reduce the bucket even with one rank (the captured-exchange path on one GPU)
        self._force_exchange = False
        # several ranks, two-layer fused step: the bucket's early part is all-reduced between the
        # step's two parts while part 2 runs on a forked stream (split_finalize), the rest after
        self._xsplit = False
        self._comm = None
        # False while the graphs hold no collective (several ranks, the exchange between graphs):
        # the whole bucket then goes in one eager all-reduce after each replay
        self._early_ok = True
        if self.world > 1:
            self._set_exchange_split()
        self.epoch = -1
        self.set_epoch(0)

    def _setup_module_slot(self, s):
        """the module path's per-slot sampler outputs: with the typed first layer
        (mag.REGNN._typed_first_layer) the last hop runs meta-only and layer 0 reads its block
        through the per-edge source type / table row; the last layer (hop 0's block)
        differentiates through a gather over that block's transposed index
        (regnn_ns_spmm_bwd_csc: no float atomics into the source rows' gradient)."""
        if self._module_lean:
            last = len(s.sizes_k) - 1
            et, eo = s.enable_edge_meta(self.local_node_idx, last)
            s.meta_only[last] = True
            blk = s.blocks[last]
            blk.edge_meta, blk.meta_only = (et, eo), True
            self._module_pre_sums(s, last)
        for h, blk in enumerate(s.blocks):
            blk.live_rows = s.sizes[h:h + 1]      # the block's live target rows (device count)
        if self._gat_blocks:
            # ops.ns_gat reads every hop in the CSR layout and differentiates by atomics
            # (regnn_ns_gat_bwd form (b)): no strided hop, no sampler index, no input sums; with
            # ops.NS_GAT_SRC "gather" by a gather over each block's own index (form (a))
            for h, blk in enumerate(s.blocks):
                blk.live_src = s.sizes[h + 1:h + 2]   # its live source rows (REGATConv's GEMMs)
            if self._gat_src_gather:
                from . import ops as _ops
                for h, blk in enumerate(s.blocks):
                    s.tidx[h] = blk.tidx = _ops.NsTidx(blk.n_dst, blk.n_src, blk.csr_idx.numel(),
                                                       self.device)
            return
        if s.blocks[0].csr_idx.numel() <= 32768:
            _, cptr, cent, clong = s.csc[0] or s.enable_csc(0)
            b0 = s.blocks[0]
            # the gather sums floats in entry order and the build's order inside a source's
            # segment follows an integer atomic: _sample sorts every segment into `csorted`
            # (regnn_ns_csc_sort), which is what the layer reads -- the same gradient bits on
            # every run of a batch
            s.csc_sorted = csorted = torch.zeros_like(cent)
            b0.csc, b0.csc_cap = (cptr, csorted, clong, s.sizes, 1), s.caps[1]
            from . import ops as _ops
            # (the layer's backward must take the transposed-index gather: ops._NsSpmm)
            if (MODULE_STRIDED["mode"] != "off" and _ops.NS_CSC["mode"] != "off" and
                    len(s.sizes_k) > 1 and
                    getattr(self.model, "hidden_dim", 0) in _ops._CSC_WIDTHS):
                # hop 0 in the strided layout (sampling + placement in one launch, the one-pass
                # de-duplication, the multi-block transposed index): its forward aggregation
                # reads rows at i S (regnn_ns_spmm_strided_fwd), its backward the index
                s.hop_strided[0] = True
                b0.strided_rows = (s.hop_bufs[0]["scnt"], s.sizes_k[0] + 1)

    def _module_bf16_unsupported(self, s):
        """why the module path cannot train on this trainer's bf16 input tables (None: it can):
        layer 0 must read the sampler's per-type input sums (_module_pre_sums) and nothing else
        may read the raw rows. The sums launch takes <= 4 tables of width 128, or with
        ops.NS_SUMS_KT "on" of one width per type, each 64 / 128 / 256."""
        m = self.model
        if getattr(m, "feats_type", 3) == 2:
            return "feats_type 2 (tables that learn) takes fp32 tables only"
        if _ops_bf16_rows_on():
            return self._bf16_rows_unsupported()
        if not self._blocks_ok:
            return ("the model does not run on device blocks (regcn, self_loop_type 2; "
                    "device_blocks=True: regat / regatv2, self_loop_type 1 / 3)")
        if any(bool(getattr(c, "residual", False)) for c in m.convs):
            return ("the module path's residual convs project the raw rows (group_input), which "
                    "reads fp32 tables")
        if MODULE_LEAN_HOP["mode"] == "off" or MODULE_PRE_SUMS["mode"] == "off":
            return "MODULE_LEAN_HOP / MODULE_PRE_SUMS is off"
        tabs = getattr(m, "_type_tables", lambda _x: None)(self.x_dict)
        if not tabs or any(t is None for t in tabs):
            return "x_dict keys must be the node types 0..T-1"
        if any(t.dtype != torch.bfloat16 for t in tabs):
            return "the tables must share one dtype"
        from . import ops as _ops
        wide = (128,) if not _ops.ns_sums_kt_on() else (64, 128, 256)
        if len(tabs) > 4 or any(t.dim() != 2 or t.shape[1] not in wide for t in tabs):
            if wide == (128,):
                return ("bf16 tables need width K = 128 and <= 4 node types (a width of 64 / "
                        "128 / 256 per type with REGNN_NS_SUMS_KT=on / ops.NS_SUMS_KT)")
            return "bf16 tables need widths of 64 / 128 / 256 and <= 4 node types"
        if not getattr(m, "typed_first_layer_ok", lambda _x: False)(self.x_dict):
            return "the typed first layer does not apply (contiguous 16-byte aligned device tables)"
        if max(s.sizes_k) > 63:
            return "a fan-out above 63"
        if not relation_slots_ok(s, len(tabs)):
            return "no relation slots (a type pair with several relations)"
        return None

    def _bf16_rows_unsupported(self):
        """_module_bf16_unsupported with ops.BF16_ROWS "on" (feats_type 2 already refused): the
        model's own readers of raw rows take all-bf16 tables -- layer 0's typed aggregation
        (ops.ns_typed_agg, where the sampler's sums do not apply) and group_input's gather-fused
        Linear (residual convs, the attention models, the exact-size path) -- so what remains is
        what those kernels cannot take: <= 8 contiguous, 16-byte aligned device tables of one
        dtype, each 64 / 128 / 256 wide, for the Linear a hidden width that is a multiple of 64."""
        from . import ops as _ops
        m = self.model
        tabs = getattr(m, "_type_tables", lambda _x: None)(self.x_dict)
        if not tabs or any(t is None for t in tabs):
            return "x_dict keys must be the node types 0..T-1"
        if any(t.dtype != torch.bfloat16 for t in tabs):
            return "the tables must share one dtype"
        Ks = [int(t.shape[1]) if t.dim() == 2 else 0 for t in tabs]
        if len(tabs) > 8 or any(K not in (64, 128, 256) for K in Ks):
            return (f"bf16 tables need widths of 64 / 128 / 256 and <= 8 node types (got "
                    f"{len(tabs)} tables of widths {Ks})")
        if not _ops.ns_typed_agg_ok(tabs):
            return "bf16 tables must be contiguous, 16-byte aligned and on the device"
        # group_input runs for every sampled row unless the typed first layer folds it in, and
        # for a residual conv's target rows
        lin = (not self._blocks_ok or self._gat_blocks or
               any(bool(getattr(c, "residual", False)) for c in m.convs) or
               not getattr(m, "typed_first_layer_ok", lambda _x: False)(self.x_dict))
        if lin:
            if getattr(m, "lins", None) is None:
                return "the model has no per-type input Linear (mag.REGNN's lins) to read them"
            Ws = [m.lins[str(k)].weight for k in range(len(tabs))]
            bs = [m.lins[str(k)].bias for k in range(len(tabs))]
            if not _ops.typed_linear_fusable(tabs, Ws, bs):
                return (f"the gather-fused Linear (ops.typed_linear) does not take hidden width "
                        f"{int(Ws[0].shape[0])}: a multiple of 64")
        return None

    def _module_pre_sums(self, s, last):
        """relation slots, <= 4 node types, inputs 128 wide -- or, with ops.NS_SUMS_KT "on", of one
        width per type, each 64 / 128 / 256 (feats_type 5's 256 / 128 / 128 / 128): the module
        path's outer hop runs as the sampler's sums launch (regnn_ns_hop_typed_sums_dt / _kt,
        strided, on the sampler's stream) and layer 0 reads the per-type sums (ops.ns_slot_agg)
        instead of gathering the sampled raw rows on the model's stream
        (mag.REGNN._typed_first_layer); hop 0 stays CSR. With the knob "off" tables of other
        widths do not qualify: layer 0 gathers their rows itself (regnn_ns_typed_agg_kt)."""
        from . import ops as _ops
        tabs = getattr(self.model, "_type_tables", lambda _x: None)(self.x_dict)
        T = len(tabs) if tabs else 0
        if (MODULE_PRE_SUMS["mode"] == "off" or not tabs or T > 4 or
                any(t is None or t.dim() != 2 for t in tabs)):
            return
        Ks = [int(t.shape[1]) for t in tabs]
        # (an equal width of 128 keeps the equal-width entry whatever the knob says; the widths
        # are settled before relation_slots_ok's pass over the graph's edges, as they were)
        kt = set(Ks) != {128}
        if kt and not (_ops.ns_sums_kt_on() and all(K in (64, 128, 256) for K in Ks)):
            return
        if (any(not t.is_contiguous() or t.data_ptr() % 16 for t in tabs) or
                max(s.sizes_k) > 63 or not relation_slots_ok(s, T)):
            return
        cap, dev = s.caps[last], self.device
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        if kt:
            U, cnt, xself = z(cap, sum(Ks)), z(cap, T), z(cap, max(Ks))
        else:
            U, cnt, xself = z(cap, T, 128), z(cap, T), z(cap, 128)
        urel = torch.full((cap, T + 1), -1, dtype=torch.int32, device=dev)
        ptrs = (ctypes.c_void_p * T)(*[t.data_ptr() for t in tabs])
        if len({t.dtype for t in tabs}) != 1:
            return
        s.typed_sums[last] = dict(tables=ptrs, dtype=L.dtype_code(tabs[0]), T=T, K=128, s_agg=U,
                                  s_w=cnt, u_self=xself,
                                  u_rel=urel, keep=tabs,
                                  # ops.ns_slot_agg and its backward read U / cnt / xself / urel
                                  # (and the block's inv) only: not the hop's per-slot meta
                                  layout=sampler_type_layout(s, T), meta_unread=True)
        if kt:
            # one width per type: run_hops then calls regnn_ns_hop_typed_sums_kt
            s.typed_sums[last]["widths"] = (ctypes.c_int32 * T)(*Ks)
            s.blocks[last].pre_widths = tuple(Ks)
        s.hop_strided[last] = True
        s.blocks[last].pre_sums = (U, cnt, xself, urel)

    # -- epochs ----------------------------------------------------------------------------------
    def steps_per_epoch(self):
        nb = -(-self.train_idx.numel() // self.sampler.B)
        return -(-nb // self.world)

    def set_epoch(self, epoch):
        """shared per-epoch permutation (every rank draws the same one: NeighborSampler's order)."""
        self.epoch = int(epoch)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed * 1_000_003 + self.epoch)
            order = torch.randperm(self.train_idx.numel(), generator=g).to(self.device)
            self.perm.copy_(self.train_idx[order])
        else:
            self.perm.copy_(self.train_idx)
        for s in self.slots:
            st = s.state
            st[0:1].fill_(_i64(self.seed))
            st[1:2].fill_(self.epoch)
            st[2:3].zero_()
        self.cur, self._primed, self._trained = 0, False, 0

    @property
    def sampler(self):
        """the sampler slot of the most recently trained batch."""
        return self.slots[self._trained]

    # -- one step --------------------------------------------------------------------------------
    def _sample(self, slot, before_sums=None):
        self._deal_targets(slot)
        self._run_hops(slot, before_sums)

    def _deal_targets(self, slot):
        """slot's next targets from the epoch permutation (its share of the round robin)."""
        n = len(self.slots)
        self.slots[slot].batch_from_perm(self.perm, self.rank + slot * self.world, n * self.world)

    def _run_hops(self, slot, before_sums=None):
        """the hops of slot's current targets, as its engine reads them."""
        s = self.slots[slot]
        if self.fused is not None:
            s.run_hops(before_sums=before_sums)
        else:                                 # the module path reads the CSR blocks
            s.run_hops(meta_only=self._module_lean, strided=False)
            if self._gat_src_gather:
                # each hop's transposed index right after the hops, on the stream that sampled
                # them: prefetched with the batch, captured with the slot's sampling
                from . import ops
                for h, blk in enumerate(s.blocks):
                    ops.ns_block_tidx(blk, out=s.tidx[h])

    def _pipelined_body(self, cur):
        """train slot `cur`'s batch while the batch of `ahead` steps later is sampled into slot
        cur + ahead (mod 2 ahead; ahead 1: the next batch into the other slot)."""
        cs = torch.cuda.current_stream(self.device)
        nxt = (cur + self.ahead) % len(self.slots)
        self._side.wait_stream(cs)
        if self.fused is None:                # the module path
            self._module_step(self.slots[cur])
            with torch.cuda.stream(self._side):
                self._sample(nxt)
            cs.wait_stream(self._side)
            return
        # the model's launches are issued (captured) before the sampler's: the graph then runs
        # the model chain on the launch queue and the sampler on the second one, and the next
        # replay's first model kernel needs no cross-queue wait (243 -> 234 us per step)
        fs = self.fused_slots[cur]
        # (the profiled eager steps of bench.py time the step as one event: unsplit)
        split = (self.ahead == 1 and fs.two_layer and SPLIT_JOIN["mode"] != "off" and
                 not profile_enabled())
        self._fs_step(fs, part=1 if split else 0)
        with torch.cuda.stream(self._side):
            self._sample(nxt)
        # the join sits between layer 1's transposed pass and layer 0's backward (the sampler is
        # done by then): the next step's first kernel then waits on its own queue only
        cs.wait_stream(self._side)
        if split:
            self._fs_step(fs, part=2)

    def _ahead_group(self, start, m, in_graph):
        """m <= ahead steps from slot `start` as one unit: the model trains slots
        start .. start + m - 1 (sampled earlier: slots cur .. cur + ahead - 1 always are) on the
        launch stream while the sampler fills slots start + ahead .. start + ahead + m - 1 (those
        trained last) on the second one; one fork before, one join after."""
        cs = torch.cuda.current_stream(self.device)
        G, n = self.ahead, len(self.slots)
        sd = self._side
        sd.wait_stream(cs)
        # "on": every step; an integer N: the sums of batches i = N, 2N, .. only (each event
        # record is a marker on the model's queue: ~4 us of queue idle between finalize and the
        # next agg0, measured in a kernel trace); "off": never
        mode = SUMS_ALIGN["mode"]
        if mode == "auto":
            s0 = self.slots[0]
            mode = "on" if (self.fused is not None and s0.strided and
                            s0.csc[0] is not None) else "2"
        every = 0 if mode == "off" or self.fused is None else (1 if mode == "on" else int(mode))
        align = every > 0
        ends = {}

        def model(i):
            if self.fused is None:             # the module path (autograd forward / backward)
                self._module_step(self.slots[(start + i) % n])
            else:
                self._fs_step(self.fused_slots[(start + i) % n])
            if in_graph:
                self._exchange()
            self._opt_step()
            if align and i + 1 < m and (i + 1) % every == 0:
                ev = torch.cuda.Event()
                ev.record(cs)
                ends[i] = ev

        def sampler(i):
            slot = (start + G + i) % n
            with torch.cuda.stream(sd):
                # batch i's outer-hop sums (the sampler's one heavy launch) wait for the end of
                # model step i - 1, so they run beside step i's agg0 / head (which they slow
                # little) instead of its gather / bwd0 / finalize (2-4x slower beside them)
                wait = ((lambda e=ends[i - 1]: sd.wait_event(e))
                        if align and i and (i - 1) in ends else None)
                self._sample(slot, before_sums=wait)

        # the model's launches first (captured first: the graph runs them on the launch queue)
        for i in range(m):
            model(i)
        for i in range(m):
            sampler(i)
        cs.wait_stream(sd)

    def _group_sizes(self):
        return group_sizes(self.ahead)

    def _advance(self):
        self._trained, self.cur = self.cur, (self.cur + 1) % len(self.slots)

    def _prime(self):
        """the sampled window ahead of slot cur: slots cur .. cur + ahead - 1."""
        if not self._primed:
            for i in range(self.ahead):
                self._sample((self.cur + i) % len(self.slots))
            self._primed = True

    def _forward_backward(self):
        if self.fused is not None:
            # every gradient is overwritten by the step (parameters the forward never reads,
            # e.g. REGNN.norm, keep the zeros of the bucket's allocation)
            if self.pipelined:
                self._prime()
                self._pipelined_body(self.cur)
                self._advance()
                return
            self._sample(0)
            self._fs_step(self.fused)
            return
        if self.pipelined:
            self._prime()
            self._pipelined_body(self.cur)
            self._advance()
            return
        self._trained = 0
        self._sample(0)
        self._module_step(self.slots[0])

    def _module_step(self, s):
        """the mag.REGNN autograd forward / nll / backward on sampler slot s's batch."""
        # the bucket zeroed once: every step overwrites each gradient the forward produces, and
        # a parameter the forward never reads (allow_unused) keeps the zeros (no fill per step)
        if not getattr(self, "_flat_zeroed", False):
            self.flat.zero_()
            self._flat_zeroed = True
        if self._gat_src_gather and not all(t is not None and t.fresh for t in s.tidx):
            raise RuntimeError("the blocks' transposed index is older than their batch (run_hops "
                               "without the index build that follows it in _sample)")
        if self._blocks_ok:
            B = s.B
            # the sampler's int32 ids as they are (torch indexes with int32; the HIP ops convert
            # where they need to): no int64 copy per step
            n_id = s.n_id
            from . import mag, ops
            fused_loss = (isinstance(self.model, mag.REGNN) and
                          os.environ.get("REGNN_NS_FUSED_LOSS", "on") != "off")
            ol = getattr(self.model, "out_lin", None)
            lin_xent = (fused_loss and LIN_XENT["mode"] != "off" and ol is not None and
                        getattr(ol, "bias", None) is not None)
            if lin_xent:
                # out_lin, the labels and the loss: ops.ns_lin_xent (forward: the GEMM and one
                # launch; backward: one launch with out_lin's bias gradient, two GEMMs)
                h = self.model(n_id, self.x_dict, s.model_blocks(), None, self.node_type,
                               self.local_node_idx, features=True)
                if h.shape[0] != B:
                    raise RuntimeError(f"the last layer has {h.shape[0]} rows, the batch {B}")
                loss = ops.ns_lin_xent(h, ol.weight, ol.bias, s.n_id, s.sizes, self.y_flat,
                                       self._xent_ticket)
            else:
                out = self.model(n_id, self.x_dict, s.model_blocks(), None, self.node_type,
                                 self.local_node_idx, **({"logits": True} if fused_loss else {}))
                # the targets' labels, -100 (ignored) past the batch's live rows: one launch
                y = ops.ns_labels(s.n_id, s.sizes, self.y_flat, B)
        else:
            # exact sizes (host sync) and the reference's (edge_index, e_id, size) adjs,
            # outermost hop first (mag/regnn_ns.py:399-403)
            n_total, hops = s.exact_adjs()
            adjs = [(ei, e_id, size) for ei, e_id, size, _blk, _cnt in hops[::-1]]
            n_id = s.n_id[:n_total].to(torch.int64)
            out = self.model(n_id, self.x_dict, adjs, self.edge_type, self.node_type,
                             self.local_node_idx)
            y = self.y_flat[n_id[:hops[0][2][1]]]
            fused_loss = lin_xent = False
        if not lin_xent:
            # log_softmax + nll in one launch each way, or the reference's pair (the mean over
            # the batch's targets)
            loss = ops.softmax_xent(out, y) if fused_loss else F.nll_loss(out, y)
        # the gradients straight into the flat bucket: autograd.grad, then one launch copying
        # every gradient (some of them transposed views) into its bucket view (backward() would
        # accumulate with one add kernel per parameter, and _foreach_copy_ / _foreach_add_
        # lower to a kernel per tensor here: ~90 us per step at hidden 512)
        seed = self._loss_seed if loss.shape == self._loss_seed.shape else None
        grads = torch.autograd.grad(loss, self.params, grad_outputs=seed, allow_unused=True)
        # the bucket is zeroed once (above), so a parameter that had a gradient on an earlier
        # step and has none now would keep the stale one: zero exactly those views (the set is
        # the same every step for a fixed model, so this is a host-side set compare only)
        had = getattr(self, "_had_grad", None)
        now = frozenset(i for i, g in enumerate(grads) if g is not None)
        if had is not None and not had <= now:
            with torch.no_grad():
                for i in had - now:
                    self.params[i].grad.zero_()
        self._had_grad = now                  # the views holding a (possibly) non-zero gradient
        with torch.no_grad():
            # (the loss rides in the same launch: no copy of its own)
            dst = [p.grad for p, g in zip(self.params, grads) if g is not None] + [self.loss]
            src = [g for g in grads if g is not None] + [loss.detach()]
            from . import ops
            ops.copy_many(dst, src)

    def _set_exchange_split(self):
        """the split exchange (two-layer fused step without the fused Adam): every slot's step
        reduces the early gradients at the end of its part 1 (regnn_nsm_work.split_finalize)."""
        if (self.fused is None or not self.fused.two_layer or self.adam_fused or
                self.n_early <= 0 or SPLIT_EXCHANGE["mode"] == "off"):
            return
        self._xsplit = True
        self._comm = torch.cuda.Stream(device=self.device)
        for fs in (self.fused_slots if self.pipelined else [self.fused]):
            fs.W.split_finalize = 1

    def _fs_step(self, fs, part=0):
        """the fused step's launches (part 0: both parts); with the split exchange, after part 1
        the early gradients' all-reduce is issued on the launch stream while part 2 runs on a
        forked stream (the collectives stay on the capture's origin stream; the next exchange
        joins the fork)."""
        if not (self._xsplit and self._early_ok):
            fs.step(part=part)
            return
        if part in (0, 1):
            fs.step(part=1)
        if part in (0, 2):
            cs = torch.cuda.current_stream(self.device)
            self._comm.wait_stream(cs)
            self._exchange_early()
            with torch.cuda.stream(self._comm):
                fs.step(part=2)

    def _exchange_early(self):
        import torch.distributed as dist
        dist.all_reduce(self.flat[:self.n_early], op=dist.ReduceOp.SUM)

    def _exchange(self):
        if self.world > 1 or self._force_exchange:
            import torch.distributed as dist
            if self._xsplit and self._early_ok:  # the early part went out after part 1
                torch.cuda.current_stream(self.device).wait_stream(self._comm)
                dist.all_reduce(self.flat[self.n_early:], op=dist.ReduceOp.SUM)
            else:
                dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
            if not isinstance(self.opt, FlatAdam):       # FlatAdam takes the mean itself
                self.flat.div_(self.world)

    def _opt_step(self):
        if not self.adam_fused:                 # else: inside the step's last launch
            self.opt.step()

    def step(self):
        """one eager step (host-launched; no host synchronisation)."""
        self._forward_backward()
        self._exchange()
        self._opt_step()

    def guarded_step(self, guard=None):
        """step() with a failure on any rank ending every rank (regnn_hip.guard): a rank whose
        forward / backward raises still issues the step's gradient all-reduce its peers are in,
        then all ranks agree on the outcome (one eager flag all-reduce) and, if any failed,
        raise guard.RankFailure together. One rank: step()."""
        from .guard import Guard
        guard = guard or Guard(self.world)
        guard.stage("NS train step", self._forward_backward, always=self._exchange)
        self._opt_step()

    def _train_state(self):
        """parameters and optimizer state, for capture() to undo its warm-up steps."""
        # (and the model's buffers: BatchNorm's running statistics move with every step)
        bufs = [b.detach().clone() for b in self.model.buffers()]
        if isinstance(self.opt, FlatAdam):
            o = self.opt
            return [t.clone() for t in (o.p, o.m, o.v, o.step_count)], None, bufs
        st = {id(p): {k: v.clone() for k, v in s.items() if torch.is_tensor(v)}
              for p, s in self.opt.state.items()}
        return [p.detach().clone() for p in self.params], st, bufs

    def _restore_train_state(self, saved):
        flat, st, bufs = saved
        with torch.no_grad():
            for b, src in zip(self.model.buffers(), bufs):
                b.copy_(src)
            if st is None:
                o = self.opt
                for dst, src in zip((o.p, o.m, o.v, o.step_count), flat):
                    dst.copy_(src)
                return
            for p, src in zip(self.params, flat):
                p.copy_(src)
            # state tensors the warm-up created (Adam: step, exp_avg, exp_avg_sq) go back to
            # their initial zeros in place: the captured graph keeps their addresses
            for p, s in self.opt.state.items():
                prev = st.get(id(p), {})
                for k, v in s.items():
                    if not torch.is_tensor(v):
                        continue
                    if k in prev:
                        v.copy_(prev[k])
                    else:
                        v.zero_()

    def capture(self, warmup=2, exchange_in_graph=None):
        """capture the step as HIP graphs: [fwd/bwd + optimizer] on one rank; [fwd/bwd] (+ the
        eager all-reduce) + [optimizer] on several. The `warmup` eager steps that precede the
        capture (kernel selection, lazy optimizer state) are undone: parameters, optimizer
        moments and step count, and the sampler's batch / edge counters are restored, so the
        first replay trains the epoch's first batch from the same model as an eager step would.
        Only the dedup stamps move on (they must stay monotone).

        exchange_in_graph (several ranks): the RCCL all-reduce and Adam are captured into the
        step's graph too, so a step is one replay with no host-issued collective and no second
        graph boundary, and runs of steps become one replay per lookahead group as with one rank.
        Default: on with an RCCL ("nccl") process group, off with gloo (a host collective cannot
        be captured); env REGNN_NS_GRAPH_ALLREDUCE=0 / 1 overrides. Measured on one GPU with the
        several-rank structure (rehearse_exchange): 157-160 us per step with the eager exchange
        between graphs, 127 us captured (125.8 one rank). A capture that fails falls back to the
        eager exchange."""
        import os
        multi = self.world > 1 or self._force_exchange
        if exchange_in_graph is None:
            env = os.environ.get("REGNN_NS_GRAPH_ALLREDUCE")
            if env is not None:
                exchange_in_graph = env == "1"
            else:
                import torch.distributed as dist
                exchange_in_graph = (multi and dist.is_available() and dist.is_initialized() and
                                     dist.get_backend() == "nccl")
        if multi and exchange_in_graph:
            saved_state = ([s.state.clone() for s in self.slots], self._train_state())
            err = None
            try:
                # capture only: nothing replays (no collective runs) until every rank agreed
                self._capture(warmup, True, warm=False)
            except RuntimeError as e:          # torch.AcceleratorError is a RuntimeError
                err = e
            # one decision for all ranks, before any replay: a rank replaying graphs with
            # captured all-reduces beside one running eager exchanges would hang the group
            if self._ranks_agree(err is None):
                self._warm_graphs()
                self.exchange_in_graph = True
                return
            import warnings
            why = f"this rank: {err}" if err is not None else "another rank's capture failed"
            warnings.warn(f"capturing the all-reduce into the step graph failed ({why}); every "
                          "rank falls back to the eager exchange between graphs")
            torch.cuda.synchronize(self.device)
            self.graphs, self.graph_groups = None, {}
            self._undo_steps(saved_state[1], saved_state[0])
            exchange_in_graph = False
        self._capture(warmup, bool(exchange_in_graph))
        self.exchange_in_graph = bool(multi and exchange_in_graph)

    def _ranks_agree(self, ok):
        """True when `ok` holds on every rank (an eager MAX all-reduce of the failure flags; one
        rank: ok itself)."""
        import torch.distributed as dist
        if self.world == 1 or not (dist.is_available() and dist.is_initialized()):
            return bool(ok)
        dev = self.device if dist.get_backend() == "nccl" else "cpu"
        flag = torch.tensor([0 if ok else 1], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        return int(flag.item()) == 0

    def _capture(self, warmup, exchange_in_graph, warm=True):
        """the eager warm-up steps (undone), then the graphs; warm: replay every multi-step
        graph once (_warm_graphs) -- capture() defers that until the ranks agreed."""
        multi = self.world > 1 or self._force_exchange
        self._early_ok = not multi or bool(exchange_in_graph)
        if self.fused is None and not self._blocks_ok:
            raise ValueError("this model's module path reads exact-size adjs (a host sync per "
                             "step) and cannot be captured; run step() eagerly")
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        st0 = [s.state.clone() for s in self.slots]
        saved = self._train_state()
        with torch.cuda.stream(side):
            for _ in range(warmup):
                # several ranks: a warm-up step that fails on one rank ends every rank together
                # (regnn_hip.guard) instead of leaving its peers in the step's all-reduce
                if multi:
                    self.guarded_step()
                else:
                    self.step()
        torch.cuda.current_stream(self.device).wait_stream(side)
        self._undo_steps(saved, st0)
        # one rank: the optimizer step joins the step's graph (no graph boundary, no host gap
        # between the backward and Adam); several: the gradient all-reduce runs between graphs,
        # or inside the graph with exchange_in_graph
        fold_opt = not multi or bool(exchange_in_graph)
        in_graph = multi and fold_opt
        if self.pipelined:
            self._prime()                      # slot 0's batch, before the first replay
            torch.cuda.synchronize(self.device)
            g1 = []
            for cur in range(len(self.slots)):   # one graph per slot
                g = torch.cuda.CUDAGraph()
                with _capturing(g):
                    # (Adam after the join: measured faster than before it, the graph then
                    # ends on one queue)
                    self._pipelined_body(cur)
                    if in_graph:
                        self._exchange()
                    if fold_opt:
                        self._opt_step()
                g1.append(g)
            self.graph_groups = {}
            if fold_opt and self.ahead > 1:
                # (m, start) -> m steps from slot start as one graph, m = ahead, ahead / 2, .. 2
                # and every start (run_steps covers any step count from any slot with few
                # replays: a run of k steps takes ~k / ahead graph boundaries and joins)
                for m in self._group_sizes():
                    for start in range(len(self.slots)):
                        g = torch.cuda.CUDAGraph()
                        with _capturing(g):
                            self._ahead_group(start, m, in_graph)
                        self.graph_groups[(m, start)] = g
            elif fold_opt and not self._gat_blocks:
                # 2 and 4 steps back to back in one graph (the slot parity returns to 0):
                # run_steps replays them for runs of steps, one graph boundary (~9 us of queue
                # idle between replays) per group instead of per step
                for n in (4, 2):
                    g = torch.cuda.CUDAGraph()
                    with _capturing(g):
                        for i in range(n):
                            self._pipelined_body(i & 1)
                            if in_graph:
                                self._exchange()
                            self._opt_step()
                    self.graph_groups[n] = g
        else:
            g1 = torch.cuda.CUDAGraph()
            with _capturing(g1):
                self._forward_backward()
                if in_graph:
                    self._exchange()
                if fold_opt:
                    self._opt_step()
        g2 = None
        if not fold_opt:
            g2 = torch.cuda.CUDAGraph()
            with _capturing(g2):
                self.opt.step()
        self.graphs = (g1, g2)
        self._cap_undo = (saved, st0, fold_opt)
        if warm:
            self._warm_graphs()

    def _warm_graphs(self):
        """every graph's first launch is slow (tens of us: the runtime's one-time work per
        executable graph); replay each once, walking the slots in training order, and undo those
        steps as the warm-up's (pipelined lookahead groups only)."""
        saved, st0, fold_opt = self._cap_undo
        self._cap_undo = None
        if self.pipelined and fold_opt and self.ahead > 1:
            g1 = self.graphs[0]
            n = len(self.slots)
            for m, start in warm_walk(self.ahead, n):
                assert start == self.cur
                (g1[start] if m == 1 else self.graph_groups[(m, start)]).replay()
                self.cur = (self.cur + m) % n
            self._undo_steps(saved, st0)

    def _undo_steps(self, saved, st0):
        """undo eager or replayed steps taken inside capture(): parameters, optimizer state,
        the sampler's batch and edge counters (not the dedup stamp, state[4]: it stays
        monotone, the tables still hold the undone steps' stamps); slot 0 .. ahead - 1 are
        sampled again by the next step (_prime)."""
        torch.cuda.synchronize(self.device)
        self._restore_train_state(saved)
        for s, s0 in zip(self.slots, st0):
            s.state[2:4].copy_(s0[2:4])
            s.state[5:6].copy_(s0[5:6])
        torch.cuda.synchronize(self.device)
        self.cur, self._primed, self._trained = 0, False, 0

    def run_steps(self, k):
        """k training steps as graph replays (capture() first), the same steps as k replay()s:
        lookahead > 1: the multi-step groups plan_run picks from any slot; lookahead 1: runs of
        4 or 2 steps from slot 0 as one graph, the rest one-step graphs."""
        k = int(k)
        groups = getattr(self, "graph_groups", {})
        if self.ahead > 1:
            n = len(self.slots)
            for m, start in plan_run(self.cur, k, self.ahead, n, lambda m, c: (m, c) in groups):
                if m == 1:
                    self.replay()
                    continue
                self._prime()
                groups[(m, start)].replay()
                self._trained, self.cur = (start + m - 1) % n, (start + m) % n
            return
        while k > 0:
            n = next((n for n in sorted(groups, reverse=True) if n <= k), 0)
            if n and self.cur == 0 and self._primed:
                groups[n].replay()
                self._trained = 1                  # slot 1's batch trained last; cur back to 0
                k -= n
            else:
                self.replay()
                k -= 1

    def replay(self):
        g1, g2 = self.graphs
        if self.pipelined:
            self._prime()                      # after set_epoch: the new epoch's first batch
            g1[self.cur].replay()
            self._advance()
        else:
            g1.replay()
        if g2 is not None:
            self._exchange()
            g2.replay()

    def rehearse_exchange(self):
        """the several-rank step structure on one rank (a timing rehearsal on one GPU, with a
        one-rank process group initialised): the bucket all-reduce after the backward and Adam
        as its own launch after it. Call before capture()."""
        self._force_exchange = True
        if self.adam_fused:
            self.adam_fused = False
            for fs in (self.fused_slots if self.pipelined else [self.fused]):
                fs.adam = None
                fs.W.adam = None
        self._set_exchange_split()

    def param_vector(self):
        """the parameters in model order without the bucket's alignment pads."""
        return torch.cat([p.detach().reshape(-1) for p in self.params])

    def edges_total(self):
        """aggregated edges of every batch sampled so far (device counters: one host sync;
        pipelined, that includes the batch sampled ahead)."""
        return int(torch.stack([s.state[5] for s in self.slots]).sum().item())
