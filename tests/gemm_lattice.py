"""The GEMM / weight-gradient lattice: one row per kernel instantiation plan_gemm / plan_wgrad can return, the inputs of a row at
an edge size M, its fp64 reference and the elementwise checker.  Shared by tests/test_gemm_lattice_cpu.py (table against the
planner, the checker against mutants of a CPU emulation) and tests/test_gemm_lattice_gpu.py (every row on the device).

The checker.  A product Y = X.W^T (+ bias + old Y + addend) computed in floating point with unit roundoff u per operation, in
ANY summation order, satisfies elementwise (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 3.5)

    |Y - ref|_ij <= c . E_ij,      E = Xabs.|W|^T + |bias| + |old Y| + |addend|      (all of it in fp64 from the fp32 inputs)

  * fp32 arithmetic (u = 2^-24): K products and K - 1 additions give gamma_K <= K u (1 + small); the lazy operand
    x = act(a.scale + shift) is itself computed in fp32 (two roundings, |error| <= 2 u (|a.scale| + |shift|) - hence
    Xabs = |a.scale| + |shift|, which also bounds |x| whatever the activation; an Rpe operand's difference and square root
    cost the same two), and the epilogue adds bias, addend, old Y and rounds the stored value (at most four more).  Together
    at most K + 8 roundings:                                    c = (K + 8) . 2^-24
    This holds for every streaming kernel and gemm_kernel / wgrad_kernel / pwgrad_kernel / pwgrad128_kernel in every mode (they
    multiply in exact fp32) and for every kernel in the fp32 mode.
  * bf16x3: split_bf16 rounds to nearest, bf16 unit roundoff v = 2^-8: a = a_hi + a_lo + r with |a_lo| <= v |a|,
    |r| <= v^2 |a|, the same for w.  The kernel sums a_hi.w_hi + a_hi.w_lo + a_lo.w_hi (exact products, fp32 accumulation): the
    dropped a_lo.w_lo and the two residual terms r_a.w, a.r_w are each <= v^2 = 2^-16 of |a.w| (second order: + O(v^3)),
                                                                c = 3 . 2^-16 + (K + 8) . 2^-24
  * bf16: a_hi.w_hi alone; |a.w - a_hi.w_hi| <= (2 v + v^2) |a.w|:  c = 2^-7 + 2^-16 + (K + 8) . 2^-24
    (the weight gradient from bf16 ROWS rounds the folded operand to bf16 as well and is held to this constant)
  * the weight gradient sums over the M rows: K -> M, and E = Xabs^T.|dY|.
On a CPU emulation a correct product sits at <= 0.2 of the fp32 bound, <= 0.45 of the bf16x3 one and ~ 0.5 of the bf16 one.
The bound is a worst case: it grows as K where the error of a correct kernel grows as sqrt(K), so at K = 512 / 1024 it has lost
most of its power against a small systematic error - the small-K rows of the same kernel family carry that burden (the mutant
tests of test_gemm_lattice_cpu.py are held at K <= 128).

Statistics, dbias and the BatchNorm-backward by-product sums keep the tolerances of test_gemm_forward, test_wgrad and
test_streaming_gemm_leaves_bn_backward_sums (tests/test_kernels_gpu.py), against the fp64 sums of the stored Y.

Rows and columns outside the product (rows beyond n in a batch-strided Y, columns beyond N where ldy > N, an operand's padding)
are pre-filled - the operand's padding with NaN, the outputs with a sentinel - and must come back bit for bit.
"""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

F32, F64 = torch.float32, torch.float64

M_GEMM = (1, 127, 129, 385)
M_WGRAD = (1, 63, 65, 257, 700)
# a concat-gather operand on the LDS-DMA wide kernel needs 16 | rows per cloud (plan_gemm_concat refuses anything else - pinned in
# test_gemm_lattice_cpu.py): the same edges, moved to the multiples of 16 on either side of the 128-row tile
M_GEMM_CAT16 = (16, 112, 144, 400)
OVERCAP = "overcap"     # M: more row tiles than the persistent grid holds workgroup rows (persistent_rows below)

# ---- the instantiations the planners can return (rl_gemm_plan / rl_wgrad_plan2 `variant`), written out ------------------------------
_MODES = ("fp32", "bf16x3", "bf16")
_W2 = [f"{k}<{m}{s},{t}>" for k in ("wgemm2_kernel", "wgemm2_cat_kernel") for m in ("bf16x3", "bf16") for s in ("", ",stats")
       for t in ("128x128", "64x128", "64x64")]
GEMM_VARIANTS = frozenset(
    [f"sgemm_kernel<{kc},{nt}>" for kc in (1, 2, 4) for nt in (1, 2, 4)] + ["sgemm_kernel<1,8>"]
    + [f"sgemm_kernel<{kc},{nt},bnb>" for kc in (1, 2, 4) for nt in (1, 2, 4)]
    + [f"sgemm_kernel<{kc},{nt},split>" for kc in (1, 2, 4) for nt in (2, 4)]
    + ["sgemm_kernel<2,1,cat>", "sgemm_kernel<4,1,cat>"]
    + [f"gemm_kernel<{nt}>" for nt in (1, 2, 4, 8)]
    + [f"pgemm_kernel<{nt},{m}>" for nt in (1, 2, 4, 8) for m in _MODES]
    + [f"wgemm_kernel<{m}{s}>" for m in ("bf16x3", "bf16") for s in ("", ",stats")]
    + _W2)
# the plans' names (rl_last_kernel) and the split-K reducers.  gemm_splitk_reduce_kernel<64> is NOT reachable: plan_gemm picks it
# when row tiles x ceil(N / 64) >= 256, and splits K only while row tiles x ceil(N / 128) < 128 - ceil(N / 64) <= 2 ceil(N / 128)
# leaves no such shape (test_gemm_lattice_cpu.py sweeps it).  Every split-K row below is reduced by <16>.
GEMM_KERNELS = frozenset(["sgemm_kernel", "sgemm_kernel<split>", "sgemm_kernel<cat>", "gemm_kernel", "pgemm_kernel", "pgemm_kernel<1>",
                          "pgemm_kernel<2>", "pgemm_kernel<4>", "pgemm_kernel<8>", "pgemm_kernel<8>+splitk", "wgemm_kernel",
                          "wgemm_kernel+splitk", "wgemm2_kernel", "wgemm2_kernel+splitk", "wgemm2_kernel<cat>"])
WGRAD_VARIANTS = frozenset(
    [f"swgrad_kernel<{kt},{nt}>" for kt in (1, 2, 4) for nt in (1, 2, 4)] + ["swgrad_kernel<1,8>"]
    + ["swgrad_cat_kernel<2,1>", "swgrad_cat_kernel<4,1>", "wgrad_kernel", "pwgrad_kernel", "pwgrad128_kernel",
       "pwgrad128w_kernel<bf16>", "pwgrad128w_kernel<bf16x3>", "pwgrad128w_kernel<bf16,bf16rows>"])


@dataclass(frozen=True)
class Case:
    id: str
    op: str                      # "gemm" | "wgrad"
    K: int
    N: int
    variant: str                 # expected plan: the instantiation ...
    kernel: str                  # ... the name rl_last_kernel reports ...
    threads: int = 256
    tile: Tuple[int, int] = (0, 0)       # ... wgemm2's tile, the K ranges, the reducer's column block
    ksplit: int = 1
    reduce_cols: int = 0
    batch: int = 0               # (wgrad) rl_wgrad_batchable
    arith: str = "fp32"          # the checker's constant
    # process settings
    mode: str = "bf16x3"
    staging: str = "dma"
    tile_setting: str = "auto"
    ksplit_setting: int = 1
    # operand facts
    planes: bool = False         # pre-split weight planes (W_split)
    lda: int = 0                 # 0: K
    misalign: bool = False       # A starts 4 bytes past a 16-byte boundary
    operand: str = "tensor"      # "tensor" | "rpe" | "cat"
    a2_first: bool = False
    rows_bf16: bool = False
    stats: bool = False
    epilogue: Optional[str] = None       # "bnb" | "dense_split" (out2 alone) | "split" (addend + out2) | "addend"
    split_col: int = 0
    Ms: tuple = ()

    @property
    def family(self) -> str:
        return self.variant.split("<")[0]


def _c(id, op, K, N, variant, kernel, **kw):
    kw.setdefault("Ms", M_GEMM if op == "gemm" else M_WGRAD)
    return Case(id, op, K, N, variant, kernel, **kw)


def _table():
    T = []
    # ---- sgemm_kernel<KC, NT>: KC from K <= 16 / 32 / 64, NT from N <= 16 / 32 / 64, <1, 8> for K <= 16 and 64 < N <= 128 ---------
    # K = 10 on lda = 12 rows (the stored relative-position rows), K % 4 != 0 with row padding (streams), full and ragged N
    S = {(1, 1): (10, 12, 13), (1, 2): (16, 0, 32), (1, 4): (6, 8, 40), (2, 1): (32, 0, 16), (2, 2): (20, 0, 24), (2, 4): (30, 32, 64),
         (4, 1): (64, 0, 2), (4, 2): (48, 0, 32), (4, 4): (64, 0, 64)}
    for (kc, nt), (K, lda, N) in S.items():
        T.append(_c(f"sgemm{kc}{nt}", "gemm", K, N, f"sgemm_kernel<{kc},{nt}>", "sgemm_kernel", lda=lda, stats=(kc + nt) % 2 == 0))
    T.append(_c("sgemm18", "gemm", 10, 128, "sgemm_kernel<1,8>", "sgemm_kernel", lda=12, stats=True))
    T.append(_c("sgemm18r", "gemm", 16, 72, "sgemm_kernel<1,8>", "sgemm_kernel"))
    # ... with the BatchNorm-backward by-product sums
    for (kc, nt), (K, lda, N) in S.items():
        T.append(_c(f"sgemm{kc}{nt}bnb", "gemm", K, N, f"sgemm_kernel<{kc},{nt},bnb>", "sgemm_kernel", lda=lda, epilogue="bnb"))
    # ... the dense split store: split_col in {16, N - 16}, and a ragged last column tile
    for kc, K, lda in ((1, 16, 0), (2, 20, 0), (4, 64, 0)):
        for nt, N, sc in ((2, 32, 16), (2, 24, 16), (4, 64, 16), (4, 64, 48), (4, 40, 16)):
            T.append(_c(f"sgemm{kc}{nt}split{N}_{sc}", "gemm", K, N, f"sgemm_kernel<{kc},{nt},split>", "sgemm_kernel<split>", lda=lda,
                        epilogue="dense_split", split_col=sc))
    # ... the concat-gather operand, both orders
    for kc, K in ((2, 32), (4, 64)):
        for first in (False, True):
            T.append(_c(f"sgemm{kc}1cat{int(first)}", "gemm", K, 16 if first else 8, f"sgemm_kernel<{kc},1,cat>", "sgemm_kernel<cat>",
                        operand="cat", a2_first=first))
    # ---- gemm_kernel<NT>: K % 4 != 0 without padding (K = 3 on lda = 3 must not stream), an unaligned tensor, the Rpe operand ----------
    T.append(_c("gemm1_k3", "gemm", 3, 8, "gemm_kernel<1>", "gemm_kernel", lda=3, stats=True))
    T.append(_c("gemm2_k10", "gemm", 10, 32, "gemm_kernel<2>", "gemm_kernel", lda=10))
    T.append(_c("gemm4_unaligned", "gemm", 64, 48, "gemm_kernel<4>", "gemm_kernel", misalign=True, stats=True))
    T.append(_c("gemm8_k90", "gemm", 90, 132, "gemm_kernel<8>", "gemm_kernel"))
    T.append(_c("gemm1_rpe", "gemm", 10, 16, "gemm_kernel<1>", "gemm_kernel", operand="rpe", stats=True))
    # ---- pgemm_kernel<NT, arithmetic>: aligned operands, no planes; K > 64 (or N > 64) keeps them off the streaming kernel --------------
    for mode in _MODES:
        for nt, K, N in ((1, 68, 12), (2, 96, 28), (4, 128, 64), (8, 40, 132)):
            T.append(_c(f"pgemm{nt}_{mode}", "gemm", K, N, f"pgemm_kernel<{nt},{mode}>", f"pgemm_kernel<{nt}>", mode=mode, arith=mode,
                        stats=nt in (2, 8)))
    # ... the split-scatter epilogue at N <= 64 and N > 64
    T.append(_c("pgemm4_split", "gemm", 128, 64, "pgemm_kernel<4,bf16x3>", "pgemm_kernel", arith="bf16x3", epilogue="split", split_col=32))
    T.append(_c("pgemm8_split", "gemm", 96, 136, "pgemm_kernel<8,bf16x3>", "pgemm_kernel<8>", arith="bf16x3", epilogue="split", split_col=68))
    T.append(_c("pgemm8_addend", "gemm", 96, 128, "pgemm_kernel<8,fp32>", "pgemm_kernel<8>", mode="fp32", epilogue="addend"))
    # ... split K (few output tiles, K >= 256): reducer <16> (see GEMM_KERNELS for <64>)
    T.append(_c("pgemm8_splitk", "gemm", 256, 128, "pgemm_kernel<8,bf16x3>", "pgemm_kernel<8>+splitk", arith="bf16x3", ksplit=4, reduce_cols=16,
                stats=True))
    T.append(_c("pgemm8_splitk_fp32", "gemm", 320, 72, "pgemm_kernel<8,fp32>", "pgemm_kernel<8>+splitk", mode="fp32", ksplit=5, reduce_cols=16))
    # ---- wgemm_kernel<arithmetic, stats>: pre-split planes where the LDS-DMA kernel does not take the operand -------------------------
    T.append(_c("wgemm_k40", "gemm", 40, 128, "wgemm_kernel<bf16x3>", "wgemm_kernel", threads=512, planes=True, arith="bf16x3"))
    T.append(_c("wgemm_k1056", "gemm", 1056, 72, "wgemm_kernel<bf16,stats>", "wgemm_kernel", threads=512, planes=True, mode="bf16", arith="bf16",
                stats=True, ksplit_setting=0))
    T.append(_c("wgemm_registers", "gemm", 128, 132, "wgemm_kernel<bf16x3,stats>", "wgemm_kernel", threads=512, planes=True, arith="bf16x3",
                stats=True, staging="registers"))
    T.append(_c("wgemm_k40_bf16", "gemm", 40, 96, "wgemm_kernel<bf16>", "wgemm_kernel", threads=512, planes=True, mode="bf16", arith="bf16"))
    T.append(_c("wgemm_splitk", "gemm", 256, 128, "wgemm_kernel<bf16x3>", "wgemm_kernel+splitk", threads=512, planes=True, arith="bf16x3",
                stats=True, staging="registers", ksplit=4, reduce_cols=16))
    # ---- wgemm2_kernel<arithmetic, stats, tile>: every tile, with and without statistics, in bf16x3 and bf16 -------------------------
    shapes = {("128", 0): (32, 128), ("128", 1): (96, 132), ("64x128", 0): (64, 132), ("64x128", 1): (160, 72),
              ("64x64", 0): (128, 200), ("64x64", 1): (224, 68)}
    for setting, tile in (("128", (128, 128)), ("64x128", (64, 128)), ("64x64", (64, 64))):
        for mode in ("bf16x3", "bf16"):
            for st in (0, 1):
                K, N = shapes[(setting, st ^ (mode == "bf16"))]
                T.append(_c(f"wgemm2_{setting}_{mode}{'_stats' if st else ''}", "gemm", K, N,
                            f"wgemm2_kernel<{mode}{',stats' if st else ''},{tile[0]}x{tile[1]}>", "wgemm2_kernel", threads=768, tile=tile,
                            planes=True, mode=mode, arith=mode, stats=bool(st), tile_setting=setting))
    # ... the narrow route (16 < N <= 64, K > 64), the K limit, split K under tile "128", and more row tiles than workgroup rows
    T.append(_c("wgemm2_narrow", "gemm", 96, 48, "wgemm2_kernel<bf16x3,stats,64x64>", "wgemm2_kernel", threads=768, tile=(64, 64), planes=True,
                arith="bf16x3", stats=True))
    T.append(_c("wgemm2_k1024", "gemm", 1024, 128, "wgemm2_kernel<bf16x3,64x64>", "wgemm2_kernel", threads=768, tile=(64, 64), planes=True,
                arith="bf16x3"))
    T.append(_c("wgemm2_splitk", "gemm", 256, 128, "wgemm2_kernel<bf16x3,128x128>", "wgemm2_kernel+splitk", threads=768, tile=(128, 128),
                planes=True, arith="bf16x3", stats=True, tile_setting="128", ksplit=4, reduce_cols=16))
    T.append(_c("wgemm2_overcap", "gemm", 32, 1024, "wgemm2_kernel<bf16x3,stats,64x64>", "wgemm2_kernel", threads=768, tile=(64, 64), planes=True,
                arith="bf16x3", stats=True, tile_setting="64x64", Ms=(OVERCAP,)))
    # ... the split-scatter epilogue on the wide kernels with planes (what the network's pooling backward runs)
    T.append(_c("wgemm2_split", "gemm", 128, 136, "wgemm2_kernel<bf16x3,64x64>", "wgemm2_kernel", threads=768, tile=(64, 64), planes=True,
                arith="bf16x3", epilogue="split", split_col=68))
    T.append(_c("wgemm_split", "gemm", 96, 128, "wgemm_kernel<bf16>", "wgemm_kernel", threads=512, planes=True, mode="bf16", arith="bf16",
                staging="registers", epilogue="split", split_col=64))
    # ... the concat-gather operand: the three tiles in both arithmetics with and without statistics, both orders on every tile
    for setting, tile in (("128", (128, 128)), ("64x128", (64, 128)), ("64x64", (64, 64))):
        for mi, mode in enumerate(("bf16x3", "bf16")):
            for st in (0, 1):
                first = (mi + st) % 2 == 1
                T.append(_c(f"wgemm2cat_{setting}_{mode}{'_stats' if st else ''}", "gemm", 64 if first else 128, 132 if st else 128,
                            f"wgemm2_cat_kernel<{mode}{',stats' if st else ''},{tile[0]}x{tile[1]}>", "wgemm2_kernel<cat>", threads=768, tile=tile,
                            planes=True, mode=mode, arith=mode, stats=bool(st), tile_setting=setting, operand="cat", a2_first=first,
                            Ms=M_GEMM_CAT16))
    # ---- the weight gradient ------------------------------------------------------------------------------------------------------
    for (kt, nt), (K, lda, N) in S.items():
        T.append(_c(f"swgrad{kt}{nt}", "wgrad", K, N, f"swgrad_kernel<{kt},{nt}>", "swgrad_kernel", lda=lda, batch=2))
    T.append(_c("swgrad18", "wgrad", 10, 128, "swgrad_kernel<1,8>", "swgrad_kernel", lda=12, batch=2))
    for kt, K in ((2, 32), (4, 64)):
        for first in (False, True):
            T.append(_c(f"swgrad{kt}1cat{int(first)}", "wgrad", K, 8 if first else 16, f"swgrad_cat_kernel<{kt},1>", "swgrad_kernel<cat>",
                        operand="cat", a2_first=first, batch=2))
    T.append(_c("swgrad11_rpe", "wgrad", 10, 16, "swgrad_kernel<1,1>", "swgrad_kernel", operand="rpe"))
    T.append(_c("wgrad_k90", "wgrad", 90, 96, "wgrad_kernel", "wgrad_kernel"))
    T.append(_c("wgrad_unaligned", "wgrad", 128, 64, "wgrad_kernel", "wgrad_kernel", misalign=True))
    T.append(_c("pwgrad_96", "wgrad", 96, 96, "pwgrad_kernel", "pwgrad_kernel"))
    T.append(_c("pwgrad128_fp32", "wgrad", 96, 128, "pwgrad128_kernel", "pwgrad128_kernel", mode="fp32"))
    T.append(_c("pwgrad128w_bf16", "wgrad", 128, 128, "pwgrad128w_kernel<bf16>", "pwgrad128w_kernel", threads=512, mode="bf16", arith="bf16", batch=1))
    T.append(_c("pwgrad128w_bf16x3", "wgrad", 256, 64, "pwgrad128w_kernel<bf16x3>", "pwgrad128w_kernel", threads=512, arith="bf16x3", batch=1))
    T.append(_c("pwgrad128w_ragged", "wgrad", 160, 132, "pwgrad128w_kernel<bf16x3>", "pwgrad128w_kernel", threads=512, arith="bf16x3", batch=1))
    T.append(_c("pwgrad128w_bf16rows", "wgrad", 128, 72, "pwgrad128w_kernel<bf16,bf16rows>", "pwgrad128w_kernel", threads=512, arith="bf16",
                rows_bf16=True))
    for first in (False, True):
        T.append(_c(f"pwgrad128w_cat{int(first)}", "wgrad", 96 if first else 160, 128 if first else 36,
                    f"pwgrad128w_kernel<{'bf16' if first else 'bf16x3'}>", "pwgrad128w_kernel", threads=512, mode="bf16" if first else "bf16x3",
                    arith="bf16" if first else "bf16x3", operand="cat", a2_first=first, batch=1))
    return T


CASES = _table()
assert len({c.id for c in CASES}) == len(CASES)


def persistent_rows(cus: int, ny: int) -> int:
    """persistent_grid's cap: the workgroup rows of a wgemm2 launch with ny column tiles on a device with `cus` compute units."""
    return max(8, cus // ny // 8 * 8)


def case_Ms(case: Case, cus: int = 256):
    """The M edges of a row; OVERCAP becomes two row tiles (and a ragged rest) more than the persistent grid's rows."""
    out = []
    for M in case.Ms:
        if M == OVERCAP:
            ny = -(-case.N // case.tile[1])
            M = (persistent_rows(cus, ny) + 2) * case.tile[0] + 37
        out.append(M)
    return out


# ---- the options, rotated over (row, M index) so that every value meets every row -----------------------------------------------------
@dataclass(frozen=True)
class Opts:
    w_n_contig: bool             # weight orientation: (K, N) storage, w_ns = 1 (else (N, K), w_ks = 1)
    bias: bool
    accumulate: bool
    lazy: Optional[int]          # None: a plain operand; else the activation 0 / 1 / 2 of a lazy one
    a_bstride: bool              # A with a batch stride (n < n_parent)
    y_bstride: bool              # Y / dY with a batch stride and a leading dimension beyond N
    pivot: bool                  # statistics around a pivot
    dbias: bool


def options(i: int, j: int) -> Opts:
    return Opts(w_n_contig=(i + j) % 2 == 1, bias=(i + j // 2) % 2 == 0, accumulate=(i // 2 + (j + 1) // 2) % 2 == 1,
                lazy=(None, 0, 1, 2)[(i // 2 + j) % 4], a_bstride=(j % 4 in (1, 2)) != (i % 2 == 1),
                y_bstride=(j % 4 in (2, 3)) != (i % 4 >= 2), pivot=j % 2 == i % 2, dbias=(i + j) % 3 != 0)


def split_rows(M: int, mult: int = 1):
    """(B, n) with B * n == M: more than one cloud where M factors (n a multiple of `mult`)."""
    for B in (2, 3, 5, 7):
        if M % B == 0 and (M // B) % mult == 0:
            return B, M // B
    return 1, M


def coefficient(arith: str, length: int) -> float:
    base = (length + 8) * 2.0 ** -24
    return {"fp32": base, "bf16x3": 3 * 2.0 ** -16 + base, "bf16": 2.0 ** -7 + 2.0 ** -16 + base}[arith]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
@dataclass
class Inputs:
    case: Case
    M: int
    opts: Opts
    B: int
    n: int
    t: dict = field(default_factory=dict)       # the tensors, by name


def _act(z, act, slope):
    if act == 1:
        return torch.relu(z)
    if act == 2:
        return torch.where(z > 0, z, z * slope)
    return z


def _rows(gen, B, n, bstride, C, ld, misalign, dtype=F32):
    """(B * bstride, ld) storage whose logical rows are the first n of each cloud and first C columns; everything else NaN."""
    rows = B * bstride
    buf = torch.full((rows * ld + 8,), float("nan"), dtype=F32)
    off = 1 if misalign else 0
    t = buf[off:off + rows * ld].view(rows, ld)
    t.view(B, bstride, ld)[:, :n, :C] = torch.randn(B, n, C, generator=gen)
    if dtype != F32:
        t = t.to(dtype).contiguous()
    return t


SLOPE = 0.2


def make_inputs(case: Case, i: int, j: int, M: int, device="cpu") -> Inputs:
    """Row `case` (index i in CASES) at its j-th edge M: every tensor of the launch, made on the host from a seed of (i, j)."""
    o = options(i, j)
    gen = torch.Generator().manual_seed(1000 * i + j)
    K, N = case.K, case.N
    cat, rpe = case.operand == "cat", case.operand == "rpe"
    wide_cat = cat and case.op == "gemm" and case.tile != (0, 0)
    t = {}
    if rpe:
        k = next(k for k in (5, 3, 1) if M % k == 0)
        B, n = split_rows(M // k)
        npar = n + 3
        t["xyz"] = torch.rand(B, npar, 3, generator=gen)
        t["nbr_idx"] = torch.randint(0, npar, (B, n, k), generator=gen, dtype=torch.int32)
        xj = torch.gather(t["xyz"], 1, t["nbr_idx"].long().reshape(B, n * k, 1).expand(-1, -1, 3)).reshape(B, n, k, 3)
        t["nbr_d2"] = ((t["xyz"][:, :n, None, :] - xj) ** 2).sum(-1)
        n_rows = n * k              # rows per cloud
    else:
        B, n = split_rows(M, 16 if wide_cat else 1)
        n_rows = n
    inp = Inputs(case, M, o, B, n, t)
    dt = torch.bfloat16 if case.rows_bf16 else F32
    lazy = o.lazy is not None and not rpe
    if cat:
        h = K // 2
        t["U"] = _rows(gen, B, n, n, h, h, False)                       # the direct rows: dense (ops.ConcatGather)
        npar = n + 5
        t["G"] = _rows(gen, B, npar, npar + 2, h, h + 4, False)         # the gathered table: batch stride, padded rows
        t["idx"] = torch.randint(0, npar, (M,), generator=gen, dtype=torch.int32)
        if lazy:
            for s in ("u", "g"):
                t[f"{s}_scale"], t[f"{s}_shift"] = torch.rand(h, generator=gen) + 0.5, torch.randn(h, generator=gen) * 0.3
    elif not rpe:
        lda = case.lda or K
        abs_ = n + 3 if o.a_bstride else n
        t["A"] = _rows(gen, B, n, abs_, K, lda, case.misalign, dt)
        if lazy:
            t["scale"], t["shift"] = torch.rand(K, generator=gen) + 0.5, torch.randn(K, generator=gen) * 0.3
    ybs = n_rows + 2 if o.y_bstride else n_rows
    if case.op == "gemm":
        W = torch.randn(N, K, generator=gen) / K ** 0.5
        t["W"] = W.t().contiguous() if o.w_n_contig else W
        if o.bias:
            t["bias"] = torch.randn(N, generator=gen)
        ycols = case.split_col if case.epilogue in ("dense_split", "split") else N
        ldy = ycols + ((4 if i % 2 else 1) if o.y_bstride else 0)
        t["Y0"] = torch.randn(B * ybs, ldy, generator=gen)              # the sentinel, and the old Y of an accumulating launch
        if case.epilogue in ("split", "addend"):
            t["addend"] = torch.randn(M, N, generator=gen)
        if case.epilogue in ("dense_split", "split"):
            t["out2_0"] = torch.randn(M, N - case.split_col, generator=gen)
        if case.epilogue == "bnb":
            t["bnb_Y"] = torch.randn(B * ybs, ldy, generator=gen)
            mean, var = torch.randn(N, generator=gen) * 0.1, torch.rand(N, generator=gen) + 0.5
            gamma, beta = torch.rand(N, generator=gen) + 0.5, torch.randn(N, generator=gen) * 0.2
            t["bnb_mean"], t["bnb_invstd"] = mean, torch.rsqrt(var + 1e-6)
            t["bnb_scale"] = gamma * t["bnb_invstd"]
            t["bnb_shift"] = beta - mean * t["bnb_scale"]
        if case.stats and o.pivot:
            t["piv_mean"] = torch.randn(N, generator=gen) * 0.5
            if not o.bias:
                t["piv_bias"] = torch.randn(N, generator=gen) * 0.5       # (a conv bias left out of the product)
    else:
        lddy = N + (4 if o.y_bstride else 0)
        t["dY"] = _rows(gen, B, n_rows, ybs, N, lddy, False, dt)
    for k_, v in t.items():
        t[k_] = v.to(device)
    if case.misalign:               # (a copy to the device lands on an aligned allocation: move it 4 bytes in again)
        buf = torch.empty(t["A"].numel() + 8, dtype=t["A"].dtype, device=device)
        t["A"] = buf[1:1 + t["A"].numel()].view(t["A"].shape).copy_(t["A"])
        assert t["A"].data_ptr() % 16 == 4
    return inp


def bnb_act(i: int, j: int):
    return (i + j) % 3          # the activation of the layer whose BatchNorm-backward sums ride along


# ---- fp64 references ------------------------------------------------------------------------------------------------------------------
def _logical(x, B, n, C):
    """The (B * n, C) logical rows of a (B * bstride, ld) storage."""
    bs = x.shape[0] // B
    return x.view(B, bs, x.shape[1])[:, :n, :C].reshape(B * n, C)


def operand_x(inp: Inputs):
    """(X, Xabs) in fp64: the operand's value act(a . scale + shift) and its envelope |a . scale| + |shift| (|a| where it is plain).
    An Rpe operand: [xi, xj, xi - xj, sqrt(d2)] formed in fp32 like the kernel, then widened."""
    c, o, t = inp.case, inp.opts, inp.t
    B, n, K = inp.B, inp.n, c.K

    def fold(a, scale, shift):
        a = a.double()
        if scale is None:
            return a, a.abs()
        z = a * scale.double() + shift.double()
        return _act(z, o.lazy, SLOPE), (a * scale.double()).abs() + shift.double().abs()

    if c.operand == "rpe":
        xyz, idx, d2 = t["xyz"], t["nbr_idx"], t["nbr_d2"]
        k = idx.shape[2]
        xi = xyz[:, :n, None, :].expand(B, n, k, 3)
        xj = torch.gather(xyz, 1, idx.long().reshape(B, n * k, 1).expand(-1, -1, 3)).reshape(B, n, k, 3)
        X = torch.cat([xi, xj, xi - xj, torch.sqrt(d2)[..., None]], -1).reshape(B * n * k, 10).double()
        return X, X.abs()
    if c.operand == "cat":
        h = K // 2
        u = _logical(t["U"], B, n, h)
        g = t["G"].view(B, -1, t["G"].shape[1])
        rows = torch.gather(g, 1, t["idx"].long().view(B, n, 1).expand(-1, -1, g.shape[2]))[:, :, :h].reshape(B * n, h)
        xu, au = fold(u, t.get("u_scale"), t.get("u_shift"))
        xg, ag = fold(rows, t.get("g_scale"), t.get("g_shift"))
        return (torch.cat([xg, xu], 1), torch.cat([ag, au], 1)) if c.a2_first else (torch.cat([xu, xg], 1), torch.cat([au, ag], 1))
    return fold(_logical(t["A"], B, n, K), t.get("scale"), t.get("shift"))


def weight_kn(inp: Inputs):
    """W as (K, N) fp64."""
    W = inp.t["W"].double()
    return W if inp.opts.w_n_contig else W.t()


def reference_gemm(inp: Inputs, X=None, Xabs=None):
    """(ref, envelope), both (M, N) fp64: v = X.W + bias + addend, + old Y on the columns that go to Y of an accumulating launch."""
    c, o, t = inp.case, inp.opts, inp.t
    if X is None:
        X, Xabs = operand_x(inp)
    W = weight_kn(inp)
    ref, env = X @ W, Xabs @ W.abs()
    if "bias" in t:
        ref, env = ref + t["bias"].double(), env + t["bias"].double().abs()
    if "addend" in t:
        ref, env = ref + t["addend"].double(), env + t["addend"].double().abs()
    if o.accumulate:
        ycols = t["Y0"].shape[1] if c.epilogue not in ("dense_split", "split") else c.split_col
        ycols = min(ycols, c.N)
        rows_per = inp.M // inp.B
        old = _logical(t["Y0"], inp.B, rows_per, ycols).double()
        ref, env = ref.clone(), env.clone()
        ref[:, :ycols] += old
        env[:, :ycols] += old.abs()
    return ref, env


def reference_wgrad(inp: Inputs):
    """(ref, envelope) as (K, N) fp64 and the fp64 column sums of dY."""
    X, Xabs = operand_x(inp)
    rows_per = inp.M // inp.B
    dY = _logical(inp.t["dY"], inp.B, rows_per, inp.case.N).double()
    return X.t() @ dY, Xabs.t() @ dY.abs(), dY.sum(0)


def check(got, ref, env, coef, what=""):
    """The elementwise bound; returns max error / bound (for the report) and asserts it is <= 1."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(err).all()), f"{what}: non-finite values in the result"
    bound = coef * env
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    if ratio > 1.0:
        flat = int((err / bound.clamp_min(1e-300)).argmax())
        r, col = divmod(flat, ref.shape[1])
        raise AssertionError(f"{what}: element ({r}, {col}) is off by {float(err[r, col]):.3e}, {ratio:.2f} x its bound "
                             f"{float(bound[r, col]):.3e} (got {float(got[r, col])!r}, fp64 {float(ref[r, col])!r}); "
                             f"{int((err > bound).sum())} of {err.numel()} elements exceed theirs")
    return ratio


# ---- the CPU emulation of the three arithmetics (test_gemm_lattice_cpu.py: the checker against mutants) ----------------------------------
def split_bf16(x):
    hi = x.to(torch.bfloat16).to(F32)
    return hi, (x - hi).to(torch.bfloat16).to(F32)


def emulate_product(X32, Wkn32, arith, drop_lo_hi=False):
    """X.W in fp32 accumulation with the kernels' operand arithmetic (X32 (M, K), Wkn32 (K, N), both fp32)."""
    if arith == "fp32":
        return X32 @ Wkn32
    ah, al = split_bf16(X32)
    wh, wl = split_bf16(Wkn32)
    if arith == "bf16":
        return ah @ wh
    y = ah @ wh + ah @ wl
    return y if drop_lo_hi else y + al @ wh


# ---- descriptors on dummy pointers (nothing is launched or dereferenced: the plan queries on a machine without a GPU) -----------------
_PTR = {name: 0x10000000 + 0x1000000 * k for k, name in enumerate(
    ["A", "W", "Y", "WS", "DY", "DW", "SLAB", "A2", "IDX", "ST", "X1", "X2", "X3", "X4", "KSLAB", "OUT2", "ADD", "XYZ", "ND2"])}


def _fill_a_dummy(d, inp: Inputs):
    c, o, B, n, K = inp.case, inp.opts, inp.B, inp.n, inp.case.K
    lazy = o.lazy is not None
    if c.operand == "rpe":
        k = inp.t["nbr_idx"].shape[2]
        d.a_mode, d.xyz, d.xyz_bstride, d.nbr_idx, d.nbr_d2, d.nbr_k = 1, _PTR["XYZ"], n + 3, _PTR["IDX"], _PTR["ND2"], k
        d.B, d.n, d.K = B, n, 10
        return
    d.a_mode, d.B, d.n, d.K = 0, B, n, K
    if c.operand == "cat":
        h = K // 2
        d.A, d.lda, d.a_bstride = _PTR["A"], h, n
        d.a2_split, d.A2, d.lda2, d.a2_bstride, d.a2_idx, d.a2_first = h, _PTR["A2"], h + 4, n + 7, _PTR["IDX"], int(c.a2_first)
        if lazy:
            d.in_scale, d.in_shift, d.in_act, d.in_slope = _PTR["X1"], _PTR["X2"], o.lazy, SLOPE
            d.a2_scale, d.a2_shift, d.a2_act, d.a2_slope = _PTR["X3"], _PTR["X4"], o.lazy, SLOPE
        return
    d.A, d.lda, d.a_bstride = _PTR["A"] + (4 if c.misalign else 0), c.lda or K, n + 3 if o.a_bstride else n
    if lazy:
        d.in_scale, d.in_shift, d.in_act, d.in_slope = _PTR["X1"], _PTR["X2"], o.lazy, SLOPE


def gemm_desc_dummy(H, L, inp: Inputs):
    c, o, t, N, K = inp.case, inp.opts, inp.t, inp.case.N, inp.case.K
    d = H.GemmDesc()
    _fill_a_dummy(d, inp)
    rows_per = inp.M // inp.B
    d.N, d.W = N, _PTR["W"]
    d.w_ks, d.w_ns = (N, 1) if o.w_n_contig else (1, K)
    d.bias = _PTR["X1"] + 0x100 if o.bias else None
    d.Y, d.ldy, d.y_bstride, d.accumulate = _PTR["Y"], t["Y0"].shape[1], rows_per + 2 if o.y_bstride else rows_per, int(o.accumulate)
    if c.planes:
        d.W_split = _PTR["WS"]
    if c.stats or c.epilogue == "bnb":
        d.stats = _PTR["ST"]
    if "piv_mean" in t:
        d.stats_pivot_mean = _PTR["X3"] + 0x100
    if c.epilogue == "bnb":
        d.bnb_Y, d.bnb_scale, d.bnb_shift, d.bnb_mean, d.bnb_invstd = (_PTR["OUT2"] + 0x100 * k for k in range(5))
    if c.epilogue in ("split", "addend"):
        d.addend = _PTR["ADD"]
    if c.epilogue in ("split", "dense_split"):
        d.out2, d.split_col = _PTR["OUT2"], c.split_col
    if N > 64 and c.operand == "tensor" and c.epilogue is None:         # (ops.gemm: the K-split scratch where the plan may want it)
        floats = L.rl_gemm_kslab_floats(inp.M, N, K)
        if floats > 0:
            d.kslab, d.kslab_floats = _PTR["KSLAB"], floats
    return d


def wgrad_desc_dummy(H, L, inp: Inputs):
    c, o, N, K = inp.case, inp.opts, inp.case.N, inp.case.K
    d = H.WgradDesc()
    _fill_a_dummy(d, inp)
    rows_per = inp.M // inp.B
    d.rows_bf16 = int(c.rows_bf16)
    d.N, d.dY, d.lddy, d.dy_bstride = N, _PTR["DY"], inp.t["dY"].shape[1], rows_per + 2 if o.y_bstride else rows_per
    d.dW = _PTR["DW"]
    d.w_ks, d.w_ns = (N, 1) if o.w_n_contig else (1, K)
    d.dbias = _PTR["X1"] + 0x100 if o.dbias else None
    d.slab, d.slab_floats = _PTR["SLAB"], L.rl_wgrad_slab_floats(inp.M, N, K)
    return d


def apply_settings(L, case: Case):
    assert L.rl_set_wide_gemm(case.mode.encode()) == 0
    assert L.rl_set_wgemm_staging(case.staging.encode()) == 0
    assert L.rl_set_wgemm_tile(case.tile_setting.encode()) == 0
    assert L.rl_set_gemm_ksplit(case.ksplit_setting) == 0


def restore_settings(L, mode0: bytes):
    L.rl_set_wide_gemm(mode0)
    L.rl_set_wgemm_staging(b"dma")
    L.rl_set_wgemm_tile(b"auto")
    L.rl_set_gemm_ksplit(1)


def expected_plan(case: Case) -> dict:
    if case.op == "gemm":
        return {"kernel": case.kernel, "variant": case.variant, "threads": case.threads, "tile": case.tile, "ksplit": case.ksplit,
                "reduce_cols": case.reduce_cols}
    return {"kernel": case.kernel, "variant": case.variant, "threads": case.threads, "batch": case.batch}


def plan_matches(case: Case, plan: dict, M: int):
    """The row's expected plan against a plan query's answer (H.gemm_plan / H.wgrad_plan)."""
    assert plan.get("rc") == 0, (case.id, M, plan)
    want = expected_plan(case)
    got = {k: plan[k] for k in want}
    assert got == want, f"{case.id} at M = {M}: planned {got}, the table says {want}"
    if case.op == "gemm":
        assert plan["grid"][2] == case.ksplit, (case.id, M, plan)
    else:
        # the row split: whole 64-row chunks per workgroup row, one slab each, a short last one
        rpb, ns = plan["rows_per_block"], plan["nsplit"]
        assert rpb % 64 == 0 and ns == max(1, -(-M // rpb)) and plan["grid"][0] == ns, (case.id, M, plan)

