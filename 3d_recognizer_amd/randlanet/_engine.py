"""Forward / backward schedule of the RandLA-Net hot path over the HIP kernels.

This is the host side of RandLANet.forward (reference randlanet/utils/modules.py:542-611) and
of its autograd backward, written as an explicit launch schedule: every step below is one call
into librandla_hip.so (include/rl_randlanet.h) on the current HIP stream, with no host
synchronisation, so a whole training step can be captured into one hipGraph (see bench.py).

Layout: activations are point-major / channel-last (B*n rows of C floats) instead of the
reference's (B,C,N,K); parameters stay in the reference's state_dict layout and are read in
place through strides, so nothing is converted at the boundary except the logits
((B,C,N), original point order).

Representation: the output of a SharedMLP is kept RAW (pre-BatchNorm) together with the
per-channel (scale, shift) of its BatchNorm and its activation (`_ops.Lazy`); consumers apply
them while loading.  BatchNorm therefore costs one tiny finalize kernel, not a pass over memory.

Random sampling: the permutation (modules.py:571-573) is applied once to the input rows; all
levels are prefixes of the permuted order (modules.py:587-598), read through batch strides;
fc_end runs in permuted order (it is per-point, and BatchNorm statistics are order-invariant)
and only the logits are un-permuted (modules.py:608).
"""
from dataclasses import dataclass, field
from typing import ClassVar, Dict, List, Optional

import torch

from . import _hip as H
from . import _ops as ops
from ._ops import Lazy, Rpe

BN_EPS = 1e-6       # modules.py:87, :497
BN_MOMENTUM = 0.99
# BatchNorm batch statistics as SHIFTED sums around a pivot (the previous batch's mean, see Engine.Pv): var = E[(y-c)^2] -
# E[y-c]^2 keeps the variance of a channel whose spread is tiny against its mean, which E[y^2] - E[y]^2 on fp32 partial sums
# loses.  A test hook (plain sums when False), not a switch
BN_PIVOT = True
# clouds below this size keep the permutation as drawn (a level-0 table of < 128 KB sits in L2 / L1 whatever the order)
BAND_SORT_MIN_POINTS = 4096
# the un-fused pooling block reads its concat operand X in place (never stored, _pool_x_in_place) only above this many rows
# (points x K); at or below it X is built once and read back as ever.  Two reasons, both stated:
#  * measured (captured train step, stored -> in place, profiles/r08_pool256_x_in_place.md section 5): 2048 rows is the one size
#    that loses (1.6070 -> 1.6091 ms, +0.13 % at a spread of 0.04 %); 3072 rows and everything above gains or ties (3072: -2.9 %,
#    4096: -0.4 to -3.4 %, 8192: -0.5 %, 10240: tie, 20480: -0.3 %, 81920: -0.9 %).  Nothing below 2048 rows was measured;
#  * the launch schedules pinned in tests/golden/step_trace.json (tests/test_schedule_gpu.py, cases A and E: 2048 rows at
#    d = 256) are the stored path's.  Without a bound those blocks would launch rl_gemm / rl_attpool_*_cat in place of
#    rl_copy_rows_pair and the recorded trace would have to be regenerated; with it they run what was recorded.
# The rule the path was specified by names no size, so this is a deviation from it: blocks of 2048 rows and fewer store X although
# the kernels would take them.  Tests set the bound to 0 to run smaller shapes in place.
POOL_X_IN_PLACE_MIN_ROWS = 2048
# a decoder step reads its concat [act(bn(x))[nn] | skip] in place (never stored, _decoder_cat_in_place) only where the concat has
# more than this many rows; at or below it the concat is built by rl_copy_rows_pair and read back as ever.  The reasons:
#  * the launch schedules and digests pinned in tests/golden/step_trace.json (tests/test_schedule_gpu.py) were recorded on the
#    stored path, and the largest decoder block of its five configurations has 8192 rows (cases A and E, decoder.3).  Above the
#    bound a step launches no rl_copy_rows_pair and its narrow input gradient no rl_copy_rows, so without the bound the recorded
#    traces would have to be regenerated; with it those configurations run what was recorded.  The bound therefore never goes
#    below 8192, whatever a measurement says;
#  * measured (captured train step with the bound at 0, profiles/r09_decoder_cat_in_place.md section 5): the configuration whose
#    largest concat has 8192 rows loses (+0.23 %); those with 16384 - 81920 rows gain 0.3 - 3 % or tie.  Nothing between 8192 and
#    16384 rows was measured.
# Blocks of 8192 rows and fewer store the concat although the kernels would take them.  Tests set the bound to 0.
DECODER_CAT_IN_PLACE_MIN_ROWS = 8192


@dataclass(slots=True, eq=False)
class _Record:
    """One step of the forward that the backward has to undo.  `level` is the encoder level the record was appended under
    (Context.record), so that the backward's launches carry the same tag in the kernel timer."""
    kind: ClassVar[str] = ""
    level: int = field(default=-1, init=False)


@dataclass(slots=True, eq=False)
class LinearRec(_Record):
    kind: ClassVar[str] = "linear"
    a: object                       # Lazy / Rpe input
    out: Lazy
    wname: str
    bname: Optional[str]
    ks: int
    ns: int
    a_grad: bool
    # this layer's dgrad product completes the gradient of its input, a BatchNorm layer's output: 1 = it is the input's only
    # consumer, 2 = the second of its two (0: neither, or not known) - see _bwd_linear
    last_consumer_of_input: int


@dataclass(slots=True, eq=False)
class PoolRec(_Record):
    kind: ClassVar[str] = "pool"
    name: str
    u: Lazy
    g: Lazy
    csr: object
    X: object                       # the stored (rows, d) tensor, or ops.ConcatGather: its halves read in place (_pool)
    S: torch.Tensor
    pooled: Lazy
    n: int
    d: int


@dataclass(slots=True, eq=False)
class PoolFusedRec(_Record):
    kind: ClassVar[str] = "pool_fused"
    name: str
    u: object                       # Lazy, or ops.VirtualRpe where stage != 0
    g: Lazy
    csr: object
    idx: torch.Tensor
    pooled: Lazy
    n: int
    d: int
    stage: int


@dataclass(slots=True, eq=False)
class AddActRec(_Record):
    kind: ClassVar[str] = "add_act"
    m2: Lazy
    sc: Lazy
    O: Lazy


@dataclass(slots=True, eq=False)
class InterpConcatRec(_Record):
    kind: ClassVar[str] = "interp_concat"
    prev: Lazy
    skip: Lazy
    csr: object
    catl: Lazy


@dataclass(slots=True, eq=False)
class HeadRec(_Record):
    kind: ClassVar[str] = "head"
    x: Lazy
    head: object
    drop: tuple


@dataclass(slots=True, eq=False)
class DropoutPhiloxRec(_Record):
    kind: ClassVar[str] = "dropout_philox"
    src: Lazy
    dropped: Lazy
    key: torch.Tensor
    p_drop: float
    seed: int
    first_row: int


@dataclass(slots=True, eq=False)
class DropoutRec(_Record):
    kind: ClassVar[str] = "dropout"
    src: Lazy
    dropped: Lazy
    mask: torch.Tensor
    scale: float


@dataclass(slots=True, eq=False)
class GradSlot:
    """The gradient of one activation tensor while the backward runs: `written` once a producer has stored into `buf` (later
    ones accumulate); `split`: the buffer holds only the interpolated half of a decoder concat's gradient, the skip half went
    to the skip tensor's slot directly (_bwd_linear)."""
    buf: torch.Tensor
    written: bool = False
    split: bool = False


class Context:
    """What one forward leaves behind for its backward, and what its own pieces hand each other."""

    def __init__(self):
        self.tape: List[_Record] = []
        self.keep: List[torch.Tensor] = []
        self.training = False
        self.B = self.N = 0
        self.perm: Optional[torch.Tensor] = None
        self.logits_perm: Optional[Lazy] = None
        self.wsplit = None                   # bf16 planes of the wide layers' weights (ops.split_weights)
        self.xyz4: Optional[torch.Tensor] = None       # coordinates padded to 16 bytes (Prep.xyz4)
        self.bn_defer: Optional[list] = None           # BatchNorm folds waiting for one grouped launch (_lfa)
        self.next_stats = (None, 1)          # batch statistics of mlp_rpe2 left by pool1's kernel (virtual rpe branch)
        self.eval_folds: Optional[dict] = None         # eval mode: the folds issued in front of the network (_eval_folds)
        self.eval_sig: Optional[tuple] = None

    def record(self, rec: _Record) -> None:
        rec.level = ops.LEVEL
        self.tape.append(rec)


class _Backward:
    """What exists only while Engine.backward runs."""

    def __init__(self, ctx: Context, grads: Dict[str, torch.Tensor]):
        self.perm, self.wsplit = ctx.perm, ctx.wsplit
        self.grads = grads                   # parameter name -> gradient tensor (the caller's)
        self.slots: Dict[object, GradSlot] = {}        # id(raw tensor) -> gradient of that activation (_key)
        self.bn_pre = {}          # raw tensor -> BatchNorm-backward partials its gradient's producer left (the fused head)
        self.bn_done = set()      # raw tensors whose BatchNorm backward already happened (fused at the residual junction)
        # backward finalizes of the virtual rpe stages wait for the next per-point layer's finalize launch and ride along with it
        # (rl_bn_bwd_finalize_batch); the stage's weight-gradient kernel, which needs the result, follows that launch (flush_rpe)
        self.fin_queue, self.rpe_after = [], []
        # weight-gradient slabs are summed by ONE launch after the last layer (they are only needed by the optimiser)
        self.pending = []
        # ... and the wide layers' weight-gradient KERNELS wait as well: one grouped launch for all of them at the end
        self.wbatch = []

    @staticmethod
    def _key(lz) -> int:
        """An activation's key: its raw tensor - or the operand itself where it is never stored (a decoder concat read in place)."""
        return id(getattr(lz, "raw", lz))

    def slot(self, lz: Lazy) -> GradSlot:
        ent = self.slots.get(self._key(lz))
        if ent is None:
            ent = self.slots[id(lz.raw)] = GradSlot(torch.empty_like(lz.raw))
        return ent

    def arrived(self, lz: Lazy) -> GradSlot:
        """The slot of a tensor whose gradient must be there by now."""
        ent = self.slot(lz)
        assert ent.written
        return ent

    def put(self, lz, buf: torch.Tensor, split: bool = False) -> None:
        self.slots[self._key(lz)] = GradSlot(buf, True, split)

    def flush_rpe(self) -> None:
        """Send out the queued backward finalizes of the virtual rpe stages (if no layer's finalize launch took them along) and
        run what waited for them."""
        if self.fin_queue:
            first = self.fin_queue.pop(0)
            ops._bn_bwd_finalize(*first, None, also=self.fin_queue)
        for fn in self.rpe_after:
            fn()
        self.rpe_after.clear()


class Prep:
    """The coordinate-only part of a forward (Engine.prepare)."""

    def __init__(self):
        self.B = self.N = 0
        self.training = False
        self.inp_p = self.xyz = self.xyz4 = None
        self.searches = self.csrs = None


class Engine:
    def __init__(self, layer_sizes, n_neighbors: int, decimation: int, n_classes: int, n_features: int,
                 params: Dict[str, torch.Tensor], buffers: Dict[str, torch.Tensor]):
        self.layers = list(layer_sizes)
        self.K = int(n_neighbors)
        self.dec = int(decimation)
        self.C = int(n_classes)
        self.F = int(n_features)
        self.P = params      # reference state_dict names -> tensors (parameters)
        self.Bf = buffers    # running_mean / running_var / num_batches_tracked
        # pivots of the shifted batch statistics, one vector per BatchNorm layer: the PREVIOUS training batch's mean of the
        # layer's output, left there by rl_bn_finalize (round 6; round 5 pivoted on the running mean, which after a
        # load_state_dict can sit ten standard deviations off the data: var = Q/n - (S/n)^2 then loses two digits).  Zero for
        # a fresh or freshly loaded model (reset_pivots): the first step runs on plain sums.  Engine state, not module state:
        # the state_dict keeps the reference's 262 / 320 entries.  Allocated HERE (a captured forward must not allocate them)
        self.Pv: Dict[str, torch.Tensor] = {k[:-len(".running_mean")]: torch.zeros_like(v) for k, v in buffers.items()
                                             if k.endswith(".running_mean")}
        # eval mode: the BatchNorm layers of a forward (name -> (C, folded conv bias)), see _fold - one table per SIGNATURE of the
        # forward (which levels run the virtual rpe branch: it folds mlp_rpe1/2's BatchNorm without the conv bias, the stored
        # branch with it, and which one a level takes depends on the batch's shape)
        self._eval_specs: Dict[tuple, dict] = {}
        self._eval_spec_build = {}
        # Dropout(fc_end): Philox mask keyed by (seed, pass counter); the counter lives on the device so that captured
        # graphs draw a new mask per replay.  The seed comes from torch's seed WITHOUT consuming its random stream.
        # data-parallel equivalence mode: BatchNorm statistics of the global batch (ops.SyncGroup)
        self.sync: Optional[ops.SyncGroup] = None
        self._drop_seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        # allocated (and zeroed) HERE, eagerly: a lazy torch.zeros inside a captured forward would become a memset node
        # of the graph and reset the counter - the same mask - on every replay
        dev = next(iter(params.values())).device
        self._drop_counter: Optional[torch.Tensor] = torch.zeros(1, dtype=torch.int64, device=dev) if dev.type == "cuda" else None
        # data-parallel runs: `drop_stream` decorrelates the masks of ranks that train on DIFFERENT batches (plain DDP:
        # the rank); `sync.first_row(N)` places a shard inside the whole batch's mask in the equivalence mode
        self.drop_stream = 0

    # ------------------------------------------------------------------------ forward pieces
    def _w2(self, name: str) -> torch.Tensor:
        w = self.P[name]
        return w.view(w.shape[0], w.shape[1])

    def _pivot(self, ctx: Context, bn_name: str):
        """The pivot of a layer's shifted batch statistics: the previous batch's mean (training only), see self.Pv."""
        if not (ctx.training and BN_PIVOT):
            return None
        return self.Pv[bn_name]

    def reset_pivots(self) -> None:
        """After the weights were replaced (load_state_dict): the pivots of the old weights' activations mean nothing."""
        for t in self.Pv.values():
            t.zero_()

    def _fold(self, ctx: Context, bn_name: str, stats, rows: int, C: int, folded_bias=None, nslots=None):
        """The BatchNorm fold of one layer (rl_bn_finalize).  Eval mode: the fold depends on nothing the forward computes (running
        statistics, gamma, beta), so the folds of ALL layers are issued in front of the network as grouped launches
        (_eval_folds: 2 launches instead of 24 dependent ones sprinkled over the chain - 6 % of an eval forward); the first
        eval forward of an engine runs them one by one and records which layers there are."""
        if not ctx.training:
            pre = ctx.eval_folds
            if pre is not None and bn_name in pre:
                scale, shift, spec_C, spec_fb = pre[bn_name]
                if spec_C == C and spec_fb is folded_bias:          # (a fold made for another path is not this layer's fold)
                    return scale, shift, None, None
            self._eval_spec_build[bn_name] = (C, folded_bias)
        nbt = self.Bf.get(f"{bn_name}.num_batches_tracked")
        return ops.bn_finalize(
            stats, rows, 128, C, self.P[f"{bn_name}.weight"], self.P[f"{bn_name}.bias"],
            self.Bf[f"{bn_name}.running_mean"], self.Bf[f"{bn_name}.running_var"],
            nbt if ctx.training else None, BN_MOMENTUM, BN_EPS, ctx.training, sync=self.sync, folded_bias=folded_bias,
            nslots=nslots, defer=ctx.bn_defer, pivoted=ctx.training and BN_PIVOT,
            pivot=self._pivot(ctx, bn_name))

    def _eval_folds(self, spec: dict):
        """(scale, shift) of every BatchNorm layer from the running statistics, as grouped launches."""
        lst, out = [], {}
        for bn_name, (C, fb) in spec.items():
            scale, shift, _, _ = ops.bn_finalize(
                None, 1, 128, C, self.P[f"{bn_name}.weight"], self.P[f"{bn_name}.bias"], self.Bf[f"{bn_name}.running_mean"],
                self.Bf[f"{bn_name}.running_var"], None, BN_MOMENTUM, BN_EPS, False, folded_bias=fb, nslots=1, defer=lst)
            out[bn_name] = (scale, shift, C, fb)
        ops.bn_finalize_flush(lst)
        return out

    def _bn(self, ctx: Context, out: Lazy, stats, bn_name: str, act: int, slope: float, folded_bias=None, nslots=None):
        scale, shift, mean, invstd = self._fold(ctx, bn_name, stats, out.rows, out.C, folded_bias, nslots)
        out.scale, out.shift, out.mean, out.invstd = scale, shift, mean, invstd
        out.act, out.slope, out.bn = act, slope, bn_name

    def _linear(self, ctx: Context, a, wname: str, bname: Optional[str], n_out: int, *, transposed=False,
                bn: Optional[str] = None, act: int = H.ACT_NONE, slope: float = 0.0, a_grad: bool = True,
                last_consumer_of_input: int = 0) -> Lazy:
        """Y = A'.W + b  (+ lazy BatchNorm/activation).  Records the layer for backward (last_consumer_of_input: see LinearRec)."""
        W = self._w2(wname)
        K = 10 if isinstance(a, Rpe) else a.C
        ks, ns = ops.weight_strides(W, transposed, K, n_out)
        stats = ops.new_stats(W.device, n_out) if (bn and ctx.training) else None
        # a bias in front of a BatchNorm cancels in (y - mean): the GEMM epilogue leaves it out (a bias costs a wide GEMM
        # launch +18 %) and the BatchNorm fold accounts for it where it shows - the running mean (rl_bn_finalize)
        fold = bn is not None and bname is not None
        piv = self._pivot(ctx, bn) if stats is not None else None
        Y = ops.gemm(a, W, ks, ns, n_out, self.P[bname] if (bname and not fold) else None, stats=stats,
                     wsplit=ctx.wsplit, pivot=(piv, self.P[bname] if fold else None) if piv is not None else None)
        rpb = a.n * a.K if isinstance(a, Rpe) else a.n
        out = Lazy(Y, a.B, rpb, rpb, n_out)
        if bn:
            self._bn(ctx, out, stats, bn, act, slope, folded_bias=self.P[bname] if fold else None,
                     nslots=ops.gemm_stat_slots(out.rows, n_out, K) if stats is not None else None)
        else:
            assert act == H.ACT_NONE
        ctx.record(LinearRec(a, out, wname, bname, ks, ns, a_grad, last_consumer_of_input))
        return out

    def _mlp_pair(self, ctx, a: Lazy, first: tuple, second: tuple, first_is_last_consumer: int = 0):
        """Two SharedMLPs over the same input (mlp1 and shortcut of an encoder level, modules.py:314, 325) as ONE wide-GEMM launch
        where rl_gemm_pair takes them; first / second: (name, n_out, act, slope).  The tape gets the two "linear" records it would
        get from two _mlp calls (the backward is theirs: `second`'s runs first, so `first` may be the last consumer of `a`)."""
        specs, metas = [], []
        for name, n_out, act, slope in (first, second):
            wname, bname, bn = f"{name}.conv.weight", f"{name}.conv.bias", f"{name}.batch_norm"
            W = self._w2(wname)
            ks, ns = ops.weight_strides(W, False, a.C, n_out)
            stats = ops.new_stats(W.device, n_out) if ctx.training else None
            piv = self._pivot(ctx, bn) if stats is not None else None
            specs.append((W, ks, ns, n_out, stats, (piv, self.P[bname]) if piv is not None else None))
            metas.append((wname, bname, bn, n_out, act, slope, ks, ns, stats))
        res = ops.gemm_pair(a, specs[0], specs[1], ctx.wsplit)
        if res is None:
            return self._mlp(ctx, a, *first, last_consumer_of_input=first_is_last_consumer), self._mlp(ctx, a, *second)
        outs = []
        for Y, (wname, bname, bn, n_out, act, slope, ks, ns, stats), last in zip(res, metas, (first_is_last_consumer, 0)):
            out = Lazy(Y, a.B, a.n, a.n, n_out)
            self._bn(ctx, out, stats, bn, act, slope, folded_bias=self.P[bname],
                     nslots=H.row_blocks(out.rows, 128) if stats is not None else None)
            ctx.record(LinearRec(a, out, wname, bname, ks, ns, True, last))
            outs.append(out)
        return outs[0], outs[1]

    def _mlp(self, ctx, a, name: str, n_out: int, act: int = H.ACT_NONE, slope: float = 0.0, *, transposed=False,
             bn=True, a_grad=True, last_consumer_of_input: int = 0) -> Lazy:
        """SharedMLP (modules.py:60-104)."""
        return self._linear(ctx, a, f"{name}.conv.weight", f"{name}.conv.bias", n_out, transposed=transposed,
                            bn=f"{name}.batch_norm" if bn else None, act=act, slope=slope, a_grad=a_grad,
                            last_consumer_of_input=last_consumer_of_input)

    def _pool(self, ctx, name: str, u, g: Lazy, idx: torch.Tensor, csr, n: int, d: int, n_out: int, stage: int = 0,
              next_stats: bool = False) -> Lazy:
        """PointFeatureAugmentation + AttentivePooling (modules.py:213-221, 246-253)."""
        B, K, h = u.B, self.K, d // 2
        rows = B * n * K
        Ws = self.P[f"{name}.score_fn.0.weight"]
        if ops.pool_supported(d, K):
            # narrow levels: one fused kernel, nothing of size rows x d touches HBM
            if next_stats:
                res, st2, ns2 = ops.pool_fwd(u, g, idx, Ws, n, d, stage, next_stats=True)
                ctx.next_stats = (st2, ns2)
            else:
                res = ops.pool_fwd(u, g, idx, Ws, n, d, stage)
            pooled = ops.plain(res, B, n)
            ctx.record(PoolFusedRec(name, u, g, csr, idx, pooled, n, d, stage))
            return self._mlp(ctx, pooled, f"{name}.mlp", n_out, H.ACT_RELU)
        # X = [act(bn(u)) | act(bn(g[idx]))] is read where its halves live - by the score product, the attentive pooling and, in
        # the backward, the weight gradient - where the library takes that operand for each of them (the d = 256 block in the
        # default arithmetic on fp32 rows with 16 neighbours, from POOL_X_IN_PLACE_MIN_ROWS rows on); else it is stored once and
        # read back.  Same bits either way.
        X = self._pool_x_in_place(ctx, u, g, idx, Ws, n, d)
        if X is None:
            X = torch.empty((rows, d), dtype=torch.float32, device=u.raw.device)
            ops.copy_rows_pair(((u.raw, (0, h), n * K, X, (0, h), rows, n * K), dict(lazy=u)),
                               ((g.raw, (0, h), g.bstride, X, (h, h), rows, n * K), dict(index=idx, lazy=g)))
            S = ops.gemm(ops.plain(X, B, n * K), Ws, 1, d, d, None, wsplit=ctx.wsplit)
        else:
            S = ops.gemm(X, Ws, 1, d, d, None, wsplit=ctx.wsplit)
        Pt = ops.attpool_fwd(X, S, B * n, K)
        pooled = ops.plain(Pt, B, n)
        ctx.record(PoolRec(name, u, g, csr, X, S, pooled, n, d))
        return self._mlp(ctx, pooled, f"{name}.mlp", n_out, H.ACT_RELU)

    def _pool_x_in_place(self, ctx, u, g: Lazy, idx: torch.Tensor, Ws: torch.Tensor, n: int, d: int):
        """The un-fused pooling block's X as an operand that is never stored (ops.ConcatGather), or None where one of its
        three readers does not take it, ops.get_pool256_x() says "stored" or the block is small (POOL_X_IN_PLACE_MIN_ROWS).  What
        the kernels support is the library's plans' to decide, not this code's."""
        K = self.K
        if (ops.get_pool256_x() != "in_place" or not isinstance(u, Lazy) or u.rows <= POOL_X_IN_PLACE_MIN_ROWS
                or u.raw.dtype != torch.float32 or g.raw.dtype != torch.float32 or ops.row_dtype() != torch.float32 or u.bstride != u.n):
            return None
        x = ops.ConcatGather(u, g, idx)
        if not ops.attpool_concat_supported(x, u.B * n, K) or not ops.gemm_concat_supported(x, Ws, 1, d, d, ctx.wsplit):
            return None
        if ctx.training and not ops.wgrad_supported(x, Ws, n * K, d):     # (Ws stands for dS, d columns of fp32: the plan reads no memory)
            return None
        return x

    def _decoder_cat_in_place(self, ctx, x: Lazy, skip: Lazy, nn: torch.Tensor, name: str, n_out: int):
        """A decoder step's concat [act(bn(x))[nn] | skip] as an operand that is never stored (ops.InterpConcat), or None
        where the step's product or weight gradient does not take it, ops.get_decoder_cat() says "stored" or the concat is small (DECODER_CAT_IN_PLACE_MIN_ROWS).  What the kernels support is the library's plans' to decide."""
        if (ops.get_decoder_cat() != "in_place" or skip.rows <= DECODER_CAT_IN_PLACE_MIN_ROWS
                or x.raw.dtype != torch.float32 or skip.raw.dtype != torch.float32 or ops.row_dtype() != torch.float32
                or skip.bstride != skip.n):
            return None
        cat = ops.InterpConcat(x, skip, nn)
        W = self._w2(f"{name}.conv.weight")
        ks, ns = ops.weight_strides(W, True, cat.C, n_out)
        if not ops.gemm_concat_supported(cat, W, ks, ns, n_out, ctx.wsplit):
            return None
        if ctx.training and not ops.wgrad_supported(cat, W, skip.n, n_out):    # (W stands for dY, n_out columns of fp32: the plan reads no memory)
            return None
        return cat

    def _virtual_bn(self, ctx: Context, vr, stage: int, bn_name: str, stats=None, nslots: int = 1) -> Lazy:
        """BatchNorm of a virtual rpe stage: statistics from rl_rpe_stats / the previous pooling kernel (training) or the
        running ones."""
        if ctx.training and stats is None:
            stats, nslots = ops.rpe_stats(vr, stage)
        scale, shift, mean, invstd = self._fold(ctx, bn_name, stats, vr.rows, vr.h, None, nslots)
        rec = Lazy(vr.d2, vr.B, vr.n * 16, vr.n * 16, vr.h, scale, shift, H.ACT_RELU, 0.0, mean, invstd, bn_name)
        return rec

    def _lfa(self, ctx, l: int, xin: Lazy, xyz: torch.Tensor, n: int, d: int, idx, d2, csr=None) -> Lazy:
        """LocalFeatureAggregation (modules.py:298-325); idx / d2 = its K nearest neighbours."""
        e = f"encoder.{l}"
        B, K, h = xin.B, self.K, d // 2
        ctx.keep += [idx, d2]
        # BatchNorm folds wanted at the same moment go out as ONE launch: (mlp1, shortcut, mlp_rpe1), then (pool1.mlp, mlp_rpe2).
        # ctx.bn_defer collects them; every flush sits in front of the first kernel that reads one of the (scale, shift) pairs
        ctx.bn_defer = [] if self.sync is None else None
        # (level 0: its input, bn_start's output, has these two consumers and no other)
        f0, sc = self._mlp_pair(ctx, xin, (f"{e}.mlp1", h, H.ACT_LRELU, 0.2), (f"{e}.shortcut", 2 * d, H.ACT_NONE, 0.0),
                                first_is_last_consumer=2 if l == 0 else 0)
        if ops.virtual_rpe_supported(d, K, B * n, n):
            # the outputs of mlp_rpe1 / mlp_rpe2 are never stored: their consumers recompute them from the coordinates
            vr = ops.VirtualRpe(ctx.xyz4 if ctx.xyz4 is not None else xyz, idx, d2, B, n, h, self.P[f"{e}.mlp_rpe1.conv.weight"], self.P[f"{e}.mlp_rpe1.conv.bias"],
                                self.P[f"{e}.mlp_rpe2.conv.weight"], self.P[f"{e}.mlp_rpe2.conv.bias"])
            vr.piv1, vr.piv2 = self._pivot(ctx, f"{e}.mlp_rpe1.batch_norm"), self._pivot(ctx, f"{e}.mlp_rpe2.batch_norm")
            vr.bn1 = self._virtual_bn(ctx, vr, 1, f"{e}.mlp_rpe1.batch_norm")
            ops.bn_finalize_flush(ctx.bn_defer)
            # in training pool1's kernel also leaves the batch statistics of mlp_rpe2's raw output (it has the tile)
            q1 = self._pool(ctx, f"{e}.pool1", vr, f0, idx, csr, n, d, h, stage=1, next_stats=ctx.training)
            vr.bn2 = self._virtual_bn(ctx, vr, 2, f"{e}.mlp_rpe2.batch_norm", *ctx.next_stats)
            ctx.next_stats = (None, 1)
            ops.bn_finalize_flush(ctx.bn_defer)
            ctx.bn_defer = None
            q2 = self._pool(ctx, f"{e}.pool2", vr, q1, idx, csr, n, d, d, stage=2)
        else:
            rpe = Rpe(xyz, idx, d2, B, n, K)
            if h <= 128:
                # read twice (forward + weight gradient): cheaper as a 48-byte row than re-gathered in both kernels, and
                # a plain 12-float row lets mlp_rpe1 run on the streaming GEMM / weight-gradient kernels (up to 128 columns)
                rpe = ops.rpe_build(rpe)
            u1 = self._mlp(ctx, rpe, f"{e}.mlp_rpe1", h, H.ACT_RELU, a_grad=False)
            ops.bn_finalize_flush(ctx.bn_defer)
            q1 = self._pool(ctx, f"{e}.pool1", u1, f0, idx, csr, n, d, h)
            u2 = self._mlp(ctx, u1, f"{e}.mlp_rpe2", h, H.ACT_RELU)
            ops.bn_finalize_flush(ctx.bn_defer)
            ctx.bn_defer = None
            q2 = self._pool(ctx, f"{e}.pool2", u2, q1, idx, csr, n, d, d)
        m2 = self._mlp(ctx, q2, f"{e}.mlp2", 2 * d, last_consumer_of_input=1)
        O = ops.plain(ops.add_act_fwd(m2, sc, 0.01), B, n)
        ctx.record(AddActRec(m2, sc, O))
        return O

    def _wide_weight_uses(self, training: bool):
        """(W, w_ks, w_ns, K, N) of every product the LDS-tiled wide GEMM will run this pass: forward orientation, and the
        dgrad orientation (strides swapped, K and N exchanged) when training."""
        uses = []
        for name, W in self.P.items():
            if not name.endswith(("conv.weight", "score_fn.0.weight")) or W.dim() < 2:
                continue
            a, b = int(W.shape[0]), int(W.shape[1])
            if max(a, b) <= 64:
                # mlp1 of a level whose shortcut is wide rides along with it (ops.gemm_pair): forward planes of the narrow weight too
                if name.endswith(".mlp1.conv.weight") and b % 32 == 0 and b > 64:
                    sc = self.P.get(name.replace(".mlp1.", ".shortcut."))
                    if sc is not None and int(sc.shape[0]) > 64:
                        uses.append((W.view(a, b), 1, b, b, a, True))
                continue
            transposed = name.startswith("decoder.")                 # ConvTranspose2d weights are (in, out)
            K, N = (a, b) if transposed else (b, a)
            ks, ns = (N, 1) if transposed else (1, K)
            W2 = W.view(a, b)
            uses.append((W2, ks, ns, K, N))
            if training:
                uses.append((W2, ns, ks, N, K))                      # dA = dY . W^T
        return uses

    # ------------------------------------------------------------------------------ forward
    def min_points(self) -> int:
        L = len(self.layers)
        return max(self.K * self.dec ** (L - 1), 2 * self.dec ** L)       # modules.py:488-491

    def prepare(self, inp: torch.Tensor, perm: torch.Tensor, training: bool) -> "Prep":
        """Everything of a forward that depends on the INPUT ROWS AND THE PERMUTATION ALONE - no weight, no activation: the
        permuted rows (modules.py:571-573), every neighbour search of the pass (the K-NN of the L encoder levels, modules.py:309,
        and the 1-NN of the L decoder steps, modules.py:358, as one batch), the padded coordinates, and - training - the transpose
        of every neighbour graph.  A caller may run this ahead of / beside the network (`_train.TrainStep`: as its own graph on a
        second stream, under the previous step's kernels) and hand the result to forward(prep=...)."""
        B, N, cin = inp.shape
        assert cin == 3 + self.F and inp.dtype == torch.float32 and inp.is_cuda and inp.is_contiguous()
        assert perm.dtype == torch.int64 and perm.numel() == N and perm.is_cuda
        assert N >= self.min_points()
        dev = inp.device
        L, dec = len(self.layers), self.dec
        prep = Prep()
        prep.B, prep.N, prep.training = B, N, training
        # random permutation of the rows (modules.py:571-573), once, on the input.  The reference sub-samples by PREFIXES of the
        # permuted order (modules.py:587-598), so only the band [N / dec^(l+1), N / dec^l) a point falls in matters; inside a band
        # the points are put in cell order, cloud by cloud (ops.band_sort: same sampled sets, neighbour gathers that follow space)
        prep.perm = perm
        edges = [0] + [N // dec ** l for l in range(L, -1, -1)]
        if (not ops.NO_BAND_SORT and N >= BAND_SORT_MIN_POINTS and len(edges) - 1 <= ops.BAND_SORT_MAX_BANDS
                and all(a < b for a, b in zip(edges[:-1], edges[1:]))):
            prep.perm = ops.band_sort(inp, perm, edges)
        inp_p = torch.empty((B * N, cin), dtype=torch.float32, device=dev)
        # coordinates padded to 16 bytes for the kernels that gather them per neighbour (virtual rpe branch) and for fc_start
        want4 = any(ops.virtual_rpe_supported(d, self.K, B * (N // dec ** l), N // dec ** l) for l, d in enumerate(self.layers))
        xyz4 = torch.empty((B, N, 4), dtype=torch.float32, device=dev) if want4 else None
        gather = dict(index=prep.perm.view(-1), index_shared=prep.perm.dim() == 1)
        if want4 and cin == 3:
            # (both from the permutation gather, one launch: the padded copy used to be a launch of its own behind the searches)
            ops.copy_rows_pair(((inp.view(B * N, 3), (0, 3), N, inp_p, (0, 3), B * N, N), gather),
                               ((inp.view(B * N, 3), (0, 3), N, xyz4.view(B * N, 4), (0, 3), B * N, N), gather))
        else:
            ops.copy_rows(inp.view(B * N, cin), (0, cin), N, inp_p, (0, cin), B * N, N, **gather)
        if cin == 3:
            xyz = inp_p.view(B, N, 3)
        else:
            xyz = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
            ops.copy_rows(inp_p, (0, 3), N, xyz.view(B * N, 3), (0, 3), B * N, N)
        prep.inp_p, prep.xyz = inp_p, xyz

        # every neighbour search of this forward depends on the coordinates only: the K-NN of the L encoder
        # levels (modules.py:309) and the 1-NN of the L decoder steps (modules.py:358) go out as one batch
        tasks, ratio = [], 1
        for _ in self.layers:
            tasks.append((N // ratio, N // ratio, self.K))
            ratio *= dec
        for _ in self.layers:
            tasks.append((N // ratio, dec * N // ratio, 1))
            ratio //= dec
        searches = ops.knn_multi(xyz, tasks)
        if want4 and cin != 3:
            ops.copy_rows(xyz.view(B * N, 3), (0, 3), N, xyz4.view(B * N, 4), (0, 3), B * N, N)
        prep.xyz4, prep.searches = xyz4, searches
        # training: the transpose of every neighbour graph ("who gathered from me"), so that the gathers' backward sums
        # each destination row in a fixed order (bitwise reproducible steps; torch's scatter_add_ has no defined order)
        prep.csrs = ops.csr_build([(searches[i][0], tasks[i][0]) for i in range(2 * L)]) if training else [None] * (2 * L)
        return prep

    def _dropout_key(self, dev):
        """(key, seed) of this pass's Dropout mask: the ticked device counter and the stream's seed."""
        if self._drop_counter is None or self._drop_counter.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise H.HipKernelError("the Dropout counter must exist before a forward is captured")
            self._drop_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        return ops.dropout_tick(self._drop_counter), (self._drop_seed + 0x9E3779B97F4A7C15 * self.drop_stream) & 0x7FFFFFFFFFFFFFFF

    def forward(self, inp: torch.Tensor, perm: torch.Tensor, training: bool, dropout_p: float = 0.5,
                keep_mask: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None,
                prep: Optional["Prep"] = None, head: Optional[ops.Head] = None):
        """inp (B,N,3+F) fp32 on the device, perm (N,) int64 on the device -> logits (B,C,N), ctx.
        keep_mask (B*N, 32) uint8: an explicit Dropout mask (parity tests); by default the mask is generated in the kernel.
        prep: the result of prepare(inp, perm, training) when the caller has run it already (same inp / perm contents).
        head (training): the labels / loss of the step - Dropout, fc_end.3, the un-permute and the loss then run as ONE kernel
        (rl_head_fwd) that fills head.out; no logits are stored and (None, ctx) is returned; backward(ctx, None, grads) starts
        from rl_head_bwd.  Without it (or where rl_head_supported says no, or for the sorted losses - lovasz, lovasz_cross_entropy -
        whose ranks need every logit of the step in memory) the layers run one by one and the logits come back."""
        B, N, cin = inp.shape
        assert cin == 3 + self.F and inp.dtype == torch.float32 and inp.is_cuda and inp.is_contiguous()
        assert perm.dtype == torch.int64 and perm.numel() == N and perm.is_cuda
        assert N >= self.min_points()
        dev = inp.device
        ctx = Context()
        ctx.training, ctx.B, ctx.N, ctx.perm = training, B, N, perm
        L, dec = len(self.layers), self.dec
        ctx.eval_sig = tuple(ops.virtual_rpe_supported(d, self.K, B * (N // dec ** l), N // dec ** l) for l, d in enumerate(self.layers))
        if not training:
            self._eval_spec_build = {}
            spec = self._eval_specs.get(ctx.eval_sig)
            if spec is not None and self.sync is None:
                ctx.eval_folds = self._eval_folds(spec)

        # wide layers: bf16 head / tail planes of their weights, both orientations, in one launch (the weights change every step)
        ctx.wsplit = ops.split_weights(self._wide_weight_uses(training))
        if prep is None:
            prep = self.prepare(inp, perm, training)
        perm = prep.perm             # (B, N) when the bands were put in cell order: what the un-permute / the head index with
        ctx.perm = perm
        assert prep.B == B and prep.N == N and prep.training >= training
        inp_p, xyz, searches, csrs = prep.inp_p, prep.xyz, prep.searches, prep.csrs
        ctx.keep += [inp_p, xyz]
        if prep.xyz4 is not None:
            ctx.keep.append(prep.xyz4)
        ctx.xyz4 = prep.xyz4

        # fc_start + bn_start (modules.py:565-566)
        # (coordinates only: the rows padded to 16 bytes - made for the virtual rpe branch - let fc_start's K = 3 product and its weight
        # gradient run on the streaming kernels, 16-byte loads, instead of the generic gemm_kernel: 18 -> 6 us at 8 clouds)
        a0 = ops.plain(inp_p, B, N)
        if cin == 3 and prep.xyz4 is not None:
            a0 = Lazy(prep.xyz4.view(B * N, 4), B, N, N, 3)
        x = self._linear(ctx, a0, "fc_start.weight", "fc_start.bias", 8, bn="bn_start.0",
                         act=H.ACT_LRELU, slope=0.2, a_grad=False)
        # encoder (modules.py:582-589)
        skips: List[Lazy] = []
        ratio = 1
        for l, d in enumerate(self.layers):
            n_l = N // ratio
            with ops.level(l):
                x = self._lfa(ctx, l, x.prefix(n_l), xyz, n_l, d, *searches[l], csr=csrs[l])
            skips.append(x)
            ratio *= dec
        x = self._mlp(ctx, x.prefix(N // ratio), "mlp", x.C, H.ACT_RELU)        # modules.py:591
        # decoder (modules.py:594-605)
        for j in range(L):
            n_c, n_f = N // ratio, dec * N // ratio
            nn = searches[L + j][0]
            assert nn.shape == (B, n_f, 1)
            skip = skips.pop()
            assert skip.n == n_f and x.n == n_c
            n_out = 8 if j == L - 1 else 2 * self.layers[L - 2 - j]
            # the concat is read where its halves live - by the step's product and, in the backward, its weight gradient - where
            # the library takes that operand for both (above DECODER_CAT_IN_PLACE_MIN_ROWS rows); else it is stored once and read
            # back.  Same bits either way.
            catl = self._decoder_cat_in_place(ctx, x, skip, nn, f"decoder.{j}", n_out)
            if catl is None:
                cat = torch.empty((B * n_f, x.C + skip.C), dtype=torch.float32, device=dev)
                ops.copy_rows_pair(((x.raw, (0, x.C), x.bstride, cat, (0, x.C), B * n_f, n_f), dict(index=nn, lazy=x)),
                                   ((skip.raw, (0, skip.C), skip.bstride, cat, (x.C, skip.C), B * n_f, n_f), {}))
                catl = ops.plain(cat, B, n_f)
                catl.concat = (x, skip)        # (backward: its gradient may leave the dgrad GEMM in two pieces, see _bwd_linear)
            ctx.record(InterpConcatRec(x, skip, csrs[L + j], catl))
            x = self._mlp(ctx, catl, f"decoder.{j}", n_out, H.ACT_RELU, transposed=True)
            ratio //= dec
        # fc_end in permuted order; the logits are un-permuted at the very end (modules.py:608-611)
        x = self._mlp(ctx, x, "fc_end.0", 64, H.ACT_RELU, last_consumer_of_input=1)
        x = self._mlp(ctx, x, "fc_end.1", 32, H.ACT_RELU, last_consumer_of_input=1)
        if (head is not None and training and self.sync is None and keep_mask is None
                and head.kind < ops.SORTED_KIND and ops.head_supported(x, self.C)):     # (a sorted loss needs the stored logits)
            key, seed, first_row = None, 0, 0
            if dropout_p > 0.0:
                key, seed = self._dropout_key(dev)
            drop = (key, seed, dropout_p, first_row)
            ops.head_fwd(x, self._w2("fc_end.3.conv.weight"), self.P["fc_end.3.conv.bias"], perm, head, drop)
            ctx.record(HeadRec(x, head, drop))
            ctx.logits_perm = None
            return None, ctx
        if training and dropout_p > 0.0:
            if keep_mask is None:
                key, seed = self._dropout_key(dev)
                first_row = self.sync.cloud_offset * N if self.sync is not None else 0
                dropped = ops.plain(ops.dropout_fwd(x, key, seed, dropout_p, first_row), B, N)
                ctx.record(DropoutPhiloxRec(x, dropped, key, dropout_p, seed, first_row))
            else:
                t = torch.empty((B * N, 32), dtype=torch.float32, device=dev)
                ops.copy_rows(x.raw, (0, 32), N, t, (0, 32), B * N, N, lazy=x)
                ops.scale_mask(t, keep_mask, 1.0 / (1.0 - dropout_p))
                dropped = ops.plain(t, B, N)
                ctx.record(DropoutRec(x, dropped, keep_mask, 1.0 / (1.0 - dropout_p)))
            x = dropped
        lp = self._mlp(ctx, x, "fc_end.3", self.C, bn=False)
        ctx.logits_perm = lp
        if not training and ctx.eval_folds is None and self._eval_spec_build:
            self._eval_specs[ctx.eval_sig] = dict(self._eval_spec_build)        # (the next eval forward of this signature folds all of them up front)
        logits = ops.logits_unpermute(lp.raw, perm, B, N, out=logits_out)
        return logits, ctx

    # ----------------------------------------------------------------------------- backward
    def backward(self, ctx: Context, dlogits: torch.Tensor, grads: Dict[str, torch.Tensor]) -> None:
        """dlogits (B,C,N) -> fills grads[name] for every parameter (reference names/layouts)."""
        if not ctx.training:
            raise H.HipKernelError("backward is implemented for training-mode forwards (batch statistics)")
        B, N = ctx.B, ctx.N
        st = _Backward(ctx, grads)
        fused_head = bool(ctx.tape) and ctx.tape[-1].kind == "head"
        if not fused_head:
            assert dlogits.shape == (B, self.C, N) and dlogits.is_cuda
            dlogits = dlogits.contiguous().float()
            st.put(ctx.logits_perm, ops.logits_permute_grad(dlogits, ctx.perm))
        for rec in reversed(ctx.tape):
            with ops.level(rec.level):
                if rec.kind != "linear":
                    st.flush_rpe()
                self._BWD[rec.kind](self, st, rec)
        st.flush_rpe()
        ops.wgrad_batch_flush(st.wbatch)
        ops.wgrad_flush(st.pending)
        ctx.tape.clear()
        ctx.keep.clear()

    def _bwd_linear(self, st: _Backward, r: LinearRec):
        a, out, wname, bname, ks, ns, grads = r.a, r.out, r.wname, r.bname, r.ks, r.ns, st.grads
        s = st.slot(out)
        assert s.written, f"no gradient reached {wname}"
        G = s.buf
        if out.scale is not None and id(out.raw) not in st.bn_done:
            ops.bn_backward(G, out, grads[f"{out.bn}.weight"], grads[f"{out.bn}.bias"], True, sync=self.sync,
                            stats=st.bn_pre.pop(id(out.raw), None), also=st.fin_queue)
            st.flush_rpe()
        n_out = out.C
        ops.wgrad(a, G, out.bstride, n_out, grads[wname], ks, ns, grads[bname] if bname else None, pending=st.pending,
                  batch=st.wbatch)
        in_place = r.a_grad and isinstance(a, ops.InterpConcat)       # a decoder concat that was never stored (_decoder_cat_in_place)
        halves = (a.x, a.skip) if in_place else getattr(a, "concat", None) if (r.a_grad and isinstance(a, Lazy)) else None
        gl = Lazy(G, out.B, out.n, out.bstride, n_out)
        # (the stored concat of a narrow step keeps its one-piece gradient: the schedules pinned for small configurations are that path's;
        # in place the plan is asked: the streaming kernel's dense split store takes K, N <= 64 where 16 | split_col)
        if (halves is not None and st._key(a) not in st.slots
                and halves[1].bstride == halves[1].n and halves[1].raw.shape[0] == a.rows
                and halves[1].raw.shape[1] == halves[1].C and halves[0].C % 4 == 0      # out2 is addressed as a dense (rows, skip.C) tensor
                and ((n_out > 64 or a.C > 64) if not in_place
                     else ops.gemm_split_supported(gl, self._w2(wname), ns, ks, a.C, halves[0].C, st.wsplit))
                and not st.slot(halves[1]).written):
            # the decoder's concat [interpolated | skip] (modules.py:362): its gradient leaves the dgrad GEMM in two pieces - the
            # interpolated half to a dense tensor (summed per coarse point by the record behind this one), the skip half
            # straight into the skip tensor's gradient, whose FIRST writer this is (the encoder's own contributions follow) -
            # instead of one (rows, C1 + C2) tensor and a strided copy of its right half
            prev, skip = halves
            gs = st.slot(skip)
            Gp = torch.empty((a.rows, prev.C), dtype=torch.float32, device=G.device)
            ops.gemm(gl, self._w2(wname), ns, ks, a.C, None, out=Gp, out_bstride=a.n if in_place else a.bstride, out2=gs.buf,
                     split_col=prev.C, wsplit=st.wsplit)
            gs.written = True
            st.put(a, Gp, split=True)
            return
        if in_place:
            # (the split store was refused: one (rows, C1 + C2) gradient, taken apart by _bwd_interp_concat)
            Ga = torch.empty((a.rows, a.C), dtype=torch.float32, device=G.device)
            ops.gemm(gl, self._w2(wname), ns, ks, a.C, None, out=Ga, out_bstride=a.n, wsplit=st.wsplit)
            st.put(a, Ga)
            return
        if r.a_grad and isinstance(a, Lazy):
            ga = st.slot(a)
            if not ga.written:
                assert a.n == a.bstride and a.raw.shape[0] == a.B * a.n, "first writer must cover the tensor"
            gl = Lazy(G, out.B, out.n, out.bstride, n_out)
            # dA = dY . W^T : the same kernel with the weight strides swapped.  Where this product COMPLETES the gradient of a
            # BatchNorm layer's output - the layer has this one consumer (fc_end.0 -> fc_end.1, the last decoder step -> fc_end.0,
            # pool2.mlp -> mlp2), or this is the second of its two (bn_start -> shortcut, then mlp1 of level 0): the forward call
            # site says so (LinearRec.last_consumer_of_input) - and the streaming kernel takes it, the layer's BatchNorm-backward
            # sums come out of the epilogue (no reduce sweep over G and Y later)
            if r.last_consumer_of_input:
                assert ga.written == (r.last_consumer_of_input == 2), wname
            complete = (bool(r.last_consumer_of_input) and self.sync is None and a.scale is not None and a.mean is not None
                        and a.rows == a.raw.shape[0])
            res = ops.gemm(gl, self._w2(wname), ns, ks, a.C, None, out=ga.buf, out_bstride=a.bstride, accumulate=ga.written,
                           wsplit=st.wsplit, bnb=a if complete else None)
            if complete and res[1] is not None:
                st.bn_pre[id(a.raw)] = res[1]
            ga.written = True

    def _bwd_pool_fused(self, st: _Backward, r: PoolFusedRec):
        if r.stage:
            return self._bwd_pool_virtual(st, r)
        u, g, n, d = r.u, r.g, r.n, r.d
        GP = st.arrived(r.pooled).buf
        gu, gg = st.slot(u), st.slot(g)
        DG = ops.pool_bwd(u, g, r.idx, self.P[f"{r.name}.score_fn.0.weight"], n, d, GP, gu.buf, gu.written,
                          st.grads[f"{r.name}.score_fn.0.weight"], pending=st.pending, batch=st.wbatch)
        gu.written = True
        # gradient of the gather: every gathered point sums its slots in a fixed order
        ops.segment_sum_rows(DG, (0, d // 2), n * self.K, r.csr, gg.buf, g.bstride, accumulate=gg.written)
        gg.written = True

    def _bwd_add_act(self, st: _Backward, r: AddActRec):
        m2, sc, O, grads = r.m2, r.sc, r.O, st.grads
        G = st.arrived(O).buf
        if ops.resid_bn_supported(m2, sc):
            # the junction's derivative and both BatchNorm backwards behind it in two sweeps
            g2 = ops.resid_bn_backward(G, O.raw, 0.01, m2, sc, grads[f"{m2.bn}.weight"], grads[f"{m2.bn}.bias"],
                                       grads[f"{sc.bn}.weight"], grads[f"{sc.bn}.bias"], sync=self.sync)
            st.bn_done.update((id(m2.raw), id(sc.raw)))
        else:
            ops.add_act_bwd(G, O.raw, 0.01)
            g2 = torch.empty_like(G)
            ops.copy_rows(G, (0, O.C), O.n, g2, (0, O.C), O.rows, O.n)
        st.put(m2, G)
        st.put(sc, g2)

    def _bwd_interp_concat(self, st: _Backward, r: InterpConcatRec):
        prev, skip, catl = r.prev, r.skip, r.catl
        s = st.arrived(catl)
        gp = st.slot(prev)
        ops.segment_sum_rows(s.buf, (0, prev.C), catl.n, r.csr, gp.buf, prev.bstride, accumulate=gp.written)
        gp.written = True
        if not s.split:              # (else: the skip half went to its gradient directly, _bwd_linear)
            gs = st.slot(skip)
            ops.copy_rows(s.buf, (prev.C, skip.C), catl.n, gs.buf, (0, skip.C), catl.rows, catl.n, accumulate=gs.written)
            gs.written = True

    def _bwd_head(self, st: _Backward, r: HeadRec):
        G, pre = ops.head_bwd(r.x, self._w2("fc_end.3.conv.weight"), self.P["fc_end.3.conv.bias"], st.perm, r.head, r.drop,
                              st.grads["fc_end.3.conv.weight"], st.grads["fc_end.3.conv.bias"], st.pending)
        st.put(r.x, G)
        if pre is not None:
            st.bn_pre[id(r.x.raw)] = pre

    def _bwd_dropout_philox(self, st: _Backward, r: DropoutPhiloxRec):
        G = st.arrived(r.dropped).buf
        ops.dropout_bwd(G, r.key, r.seed, r.p_drop, r.first_row)
        st.put(r.src, G)

    def _bwd_dropout(self, st: _Backward, r: DropoutRec):
        G = st.arrived(r.dropped).buf
        ops.scale_mask(G, r.mask, r.scale)
        st.put(r.src, G)

    def _bwd_pool_virtual(self, st: _Backward, r: PoolFusedRec):
        """Pooling block whose rpe half is virtual, followed by the backward of that stage itself (its BatchNorm + ReLU +
        Linear: mlp_rpe2 for stage 2, mlp_rpe1 for stage 1 - they have no tape records of their own)."""
        name, vr, g, n, d, stage, grads = r.name, r.u, r.g, r.n, r.d, r.stage, st.grads
        h = d // 2
        e = name.rsplit(".", 1)[0]                       # encoder.<l>
        GP = st.arrived(r.pooled).buf
        key = ("vgu", id(vr))
        if stage == 2:
            GU = torch.empty((vr.rows, h), dtype=ops.row_dtype(), device=GP.device)     # bf16 in the bf16-storage mode
            first = True
        else:
            GU, first = st.slots.pop(key).buf, False     # written by stage 2's Linear backward (dY2 . W2)
        gg = st.slot(g)
        # this launch completes GU (stage 2: its only writer; stage 1: it adds the pooling path to dY2 . W2), so it can
        # leave the batch-statistics sums of the stage's BatchNorm backward as well
        nslots = H.lib().rl_pool_bwd_slots(vr.B * n, d)
        bstats = torch.empty((nslots, 2, h), dtype=torch.float64, device=GP.device)
        DG = ops.pool_bwd(vr, g, r.idx, self.P[f"{name}.score_fn.0.weight"], n, d, GP, GU, not first,
                          grads[f"{name}.score_fn.0.weight"], pending=st.pending, stage=stage, bn_bwd_stats=bstats)
        ops.segment_sum_rows(DG, (0, h), n * self.K, r.csr, gg.buf, g.bstride, accumulate=gg.written)
        gg.written = True
        # the stage's own backward: batch-statistics terms of its BatchNorm, then weight / bias (/ input) gradients
        layer = f"{e}.mlp_rpe{stage}"
        queue = st.fin_queue if self.sync is None else None
        coef = ops.rpe_bn_backward(vr, stage, GU, grads[f"{layer}.batch_norm.weight"], grads[f"{layer}.batch_norm.bias"],
                                   sync=self.sync, stats=bstats, nslots=nslots, queue=queue)
        GU1 = torch.empty_like(GU) if stage == 2 else None

        def finish():
            with ops.level(r.level):
                ops.rpe_wgrad(vr, stage, GU, coef, grads[f"{layer}.conv.weight"], grads[f"{layer}.conv.bias"], st.pending, GU1)
        if queue is not None:
            st.rpe_after.append(finish)         # behind the finalize launch that carries this stage's sums (flush_rpe)
        else:
            finish()
        if stage == 2:
            st.slots[key] = GradSlot(GU1, True)

    def _bwd_pool(self, st: _Backward, r: PoolRec):
        name, u, g, csr, X, S, pooled, n, d, grads = r.name, r.u, r.g, r.csr, r.X, r.S, r.pooled, r.n, r.d, st.grads
        B, K, h = u.B, self.K, d // 2
        rows = B * n * K
        GP = st.arrived(pooled).buf
        dS, dX = ops.attpool_bwd(X, S, pooled.raw, GP, B * n, K)
        Ws = self.P[f"{name}.score_fn.0.weight"]
        ops.wgrad(X if isinstance(X, ops.ConcatGather) else ops.plain(X, B, n * K), dS, n * K, d,
                  grads[f"{name}.score_fn.0.weight"], 1, d, None, pending=st.pending, batch=st.wbatch)
        gu = st.slot(u)
        gg = st.slot(g)
        if d <= 64:      # the epilogue lives in the wide (LDS-tiled) kernel only
            ops.gemm(ops.plain(dS, B, n * K), Ws, d, 1, d, None, out=dX, out_bstride=n * K, accumulate=True,
                     wsplit=st.wsplit)
            ops.copy_rows(dX, (0, h), n * K, gu.buf, (0, h), rows, n * K, accumulate=gu.written)
            ops.segment_sum_rows(dX, (h, h), n * K, csr, gg.buf, g.bstride, accumulate=gg.written)
        else:
            # dX = dP*A + dS.W leaves the GEMM epilogue in two pieces: the rpe-branch half is stored (or accumulated)
            # where it belongs, the gathered half goes to a dense tensor that is then summed per gathered point
            DG = torch.empty((rows, h), dtype=torch.float32, device=dX.device)
            ops.gemm(ops.plain(dS, B, n * K), Ws, d, 1, d, None, out=gu.buf, out_bstride=n * K, accumulate=gu.written,
                     addend=dX, out2=DG, split_col=h, wsplit=st.wsplit)
            ops.segment_sum_rows(DG, (0, h), n * K, csr, gg.buf, g.bstride, accumulate=gg.written)
        gu.written = gg.written = True

    _BWD = {"linear": _bwd_linear, "pool": _bwd_pool, "pool_fused": _bwd_pool_fused, "add_act": _bwd_add_act,
            "interp_concat": _bwd_interp_concat, "head": _bwd_head, "dropout_philox": _bwd_dropout_philox,
            "dropout": _bwd_dropout}
