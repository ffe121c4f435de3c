"""The BatchNorm lattice: one row per kernel variant x layout x edge of csrc/bn.hip, the inputs of a row at an edge, the fp64
reference, the derived bounds and a numpy emulation of every kernel family's summation layout.  Shared by
tests/test_bn_lattice_cpu.py (table self-checks, host-only entry points, the emulation inside every bound, twelve mutants of
it rejected) and tests/test_bn_lattice_gpu.py (every row on the device).

Backward.  G holds d(loss)/d(activated output); with d = act'(y.scale + shift), g = G.d and xhat = (y - mean).invstd
    dbeta = sum g      dgamma = sum g.xhat      coef = (dbeta, dgamma) / count      dY = scale.(g - coef0 - xhat.coef1)
The reference evaluates exactly these expressions in fp64 (numpy) from the fp32 inputs as stored; `mean` / `invstd` are given
vectors.  The activation's sign is made unambiguous by construction: make_bwd moves every element with
|y.sc + sh| < 2^-18 (|y.sc| + |sh|) by 0.5 and asserts that none is left (an fp32 z, fused or not, is within 2^-23 of that
envelope), so the comparison leaves no element out.

Bounds, u = 2^-24, v = 2^-53.  None of them was tuned against a kernel.
  * Per-channel sums.  A term g or g.xhat is formed with at most 4 fp32 roundings (the slope, the subtraction, invstd, the
    product) and then passes through at most D fp32 additions, D from the kernel's layout (sum_depth):
        sweeps         rows per lane per tile x tiles per workgroup (+ the butterfly steps of the float4 kernels, C/4 < 64)
        one launch     SM_R rows per lane + the 6 steps of the wave sum
    Everything behind that is summed in double.  |sum - ref| <= 2 (D + 4) u sum|term| + u |sum|: the factor 2 is the stated
    margin for the second-order terms and the double sums, u |sum| the fp32 store.  coef = (float)(sum / count) gets the first
    part divided by count plus u |coef|.
  * dY, per element.  Seven roundings (g: 1, xhat: 2, xhat.coef1: 1, two subtractions, the scale), each at most u of
    E = |g| + |coef0| + |xhat.coef1|, and the error the coefficients carry in:
        |dY - ref| <= |scale| ((1 + 2^-10) 7 u E + |d coef0| + |xhat| |d coef1|)
    An apply without coefficients (activation derivative and scale only) has 2 roundings: (1 + 2^-10) 2 u |scale.g|.
  * Forward fold.  S, Q summed in double over nslots partials: dS = nslots v sum|s_i|, the same for Q.  ms = S / n,
    mean = pivot + ms (pivot: the fp32 value `running mean - folded bias` or `pivot vector - folded bias`, formed in fp32 as
    the producer of the sums formed it - an input of the fold, taken as given), var = Q / n - ms^2 clamped at 0:
        d ms = dS / n + v |ms|      d mean = d ms + v |mean|      d var = dQ / n + 2 |ms| d ms + 3 v (Q / n + ms^2)
    - the cancellation of var = Q/n - ms^2 is carried by that last term: relative to var it is 3 v (Q/n + ms^2) / var, and a
    row whose factor (Q/n + ms^2) / var exceeds 2^20 does not belong in the table (asserted; the clamp row only asserts
    var = 0 and finiteness).  invstd = (float) 1/sqrt(var + eps):  d invstd = invstd (d var / (var + eps) + 4 v + u) (the
    first-order term is half of that; the rest is the margin for its curvature).  Then the fp32 expressions, each rounding
    bounded by u times the magnitude it rounds:
        scale = g.invstd                 d scale = |g| d invstd + u |scale|
        shift = b - (float)mean.scale    d shift = |scale| (d mean + u |mean|) + |mean| d scale + u |mean.scale| + u (|b| + |mean.scale|)
        rmean = a.rm + m.((float)mean + fb), a = 1.f - m in fp32
                                         d = m (d mean + u |mean| + u |mean + fb|) + 2 u (|a.rm| + |m (mean + fb)|)
        rvar  = a.rv + m.(float)unbiased, unbiased = var n / (n - 1) (n > 1)
                                         d = m (d var n / (n - 1) + (2 v + u) unbiased) + 2 u (|a.rv| + |m.unbiased|)
        pivot = (float)mean + fb         d = d mean + u |mean| + u |mean + fb|
    all times (1 + 2^-10).  The reference sums with math.fsum and continues in extended precision.
  * rl_bn_reduce_slots: nslots v sum|x|.  The backward finalizers on given partials: the same d on the double sum, then
    d + u (|sum| + d) for the fp32 store; coef divides in double first (d / count + v |coef|).
"""
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

U, V = 2.0 ** -24, 2.0 ** -53
M2 = 1.0 + 2.0 ** -10
F32, F64 = np.float32, np.float64
MAX_SLOTS, SM_T, SM_ROWS = 1024, 1024, 2048
BNF_MAX, BNBF_MAX = 24, 8
SLOPE = 0.2
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
EPS, MOMENTUM = F32(1e-6), F32(0.99)

REDUCE_VEC, APPLY_VEC = "bn_bwd_reduce_vec_kernel", "bn_bwd_apply_vec_kernel"
REDUCE_SCALAR, APPLY_SCALAR = "bn_bwd_reduce_kernel", "bn_bwd_apply_kernel"
SMALL, RESID_REDUCE, RESID_APPLY, RESID_SMALL = ("bn_bwd_small_kernel", "resid_bn_bwd_reduce_kernel", "resid_bn_bwd_apply_kernel",
                                                 "resid_bn_bwd_small_kernel")
KERNELS = {"vec": (REDUCE_VEC, APPLY_VEC), "scalar": (REDUCE_SCALAR, APPLY_SCALAR), "small": (SMALL,),
           "resid_sweep": (RESID_REDUCE, RESID_APPLY), "resid_small": (RESID_SMALL,)}
ENTRY_POINTS = {"vec": ("rl_bn_bwd_reduce", "rl_bn_bwd_finalize", "rl_bn_bwd_finalize_pair", "rl_bn_bwd_finalize_batch", "rl_bn_bwd_apply"),
                "small": ("rl_bn_bwd_fused",), "resid_small": ("rl_resid_bn_bwd_fused",),
                "resid_sweep": ("rl_resid_bn_bwd_reduce", "rl_bn_bwd_finalize", "rl_bn_bwd_finalize_pair", "rl_bn_bwd_finalize_batch",
                                "rl_resid_bn_bwd_apply")}
ENTRY_POINTS["scalar"] = ENTRY_POINTS["vec"]
# what the suite must have seen rl_last_kernel report (the one-launch kernels at both SM_R)
REACHED = frozenset([(REDUCE_VEC, 0), (APPLY_VEC, 0), (REDUCE_SCALAR, 0), (APPLY_SCALAR, 0), (SMALL, 1), (SMALL, 2),
                     (RESID_REDUCE, 0), (RESID_APPLY, 0), (RESID_SMALL, 1), (RESID_SMALL, 2)])


# ---- the host's layout arithmetic, restated ------------------------------------------------------------------------------------------
def bn_tile(M: int) -> int:
    t = 16
    while t < 256 and t * 4096 < M:
        t <<= 1
    return t


def slots(M: int) -> int:
    return min(max(1, -(-M // bn_tile(M))), MAX_SLOTS)


def vec_eligible(C: int) -> bool:
    c4 = C >> 2
    return C % 4 == 0 and 1 <= c4 <= 256 and c4 & (c4 - 1) == 0


def lanes(family: str, C: int) -> Tuple[int, int]:
    """(tpr, rpar): lanes that sweep one row, rows in flight per workgroup."""
    tpr = min(C, 256) if family == "scalar" else min(C >> 2, 256)
    return tpr, 256 // tpr


def sm_r(M: int) -> int:
    return 1 if M <= SM_T else 2


def small_quads(C: int):
    """small_quad of every workgroup of a one-launch grid: the channel quad it owns, or -1."""
    nq, per = C >> 2, ((C >> 2) + 7) >> 3
    out = []
    for b in range(8 * per):
        q = (b & 7) * per + (b >> 3)
        out.append(q if (b >> 3) < per and q < nq else -1)
    return out


def sum_depth(family: str, C: int, M: int) -> int:
    """D: the fp32 additions a term passes through at most, as the kernel lays the rows out."""
    if family in ("small", "resid_small"):
        return sm_r(M) + 6
    tpr, rpar = lanes(family, C)
    tile = bn_tile(M)
    ntiles = -(-M // tile)
    grid = min(ntiles, MAX_SLOTS)
    butterfly = int(math.log2(64 // tpr)) if family != "scalar" and tpr < 64 else 0
    return -(-tile // rpar) * -(-ntiles // grid) + butterfly


# ---- the table -------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Edge:
    B: int
    n: int
    bstride: int

    @property
    def M(self) -> int:
        return self.B * self.n


@dataclass(frozen=True)
class Case:
    id: str
    family: str                      # "vec" | "scalar" | "small" | "resid_sweep" | "resid_small"
    C: int
    edges: Tuple[Edge, ...]
    ld: int = 0                      # 0: C
    misalign: Optional[str] = None   # "base": G and Y start 4 bytes past a 16-byte boundary; "vectors": scale and mean do

    @property
    def kernels(self):
        return KERNELS[self.family]

    @property
    def entry_points(self):
        return ENTRY_POINTS[self.family]

    @property
    def lda(self) -> int:
        return self.ld or self.C


def dense(*Ms):
    return tuple(Edge(1, M, M) for M in Ms)


STRIDED = Edge(3, 37, 50)
SMALL_ROWS = (1, 63, 64, 1023, 1024, 1025, 2047, 2048)


def row_edges(family: str, C: int):
    """1, rpar - 1, rpar, rpar + 1, 2 rpar + 1, tile - 1, tile, tile + 1 at the 16-row tile of a small tensor."""
    _, rpar = lanes(family, C)
    return tuple(sorted({M for M in (1, rpar - 1, rpar, rpar + 1, 2 * rpar + 1, 15, 16, 17) if M >= 1}))


def _table():
    T = []
    for C in (4, 8, 128, 256, 512, 1024):
        T.append(Case(f"vec_c{C}", "vec", C, dense(*row_edges("vec", C))))
    for C in (1, 3, 6, 10, 12, 100, 255, 257, 300, 1023):
        T.append(Case(f"scalar_c{C}", "scalar", C, dense(*row_edges("scalar", C))))
    # a float4-eligible C made scalar by its leading dimension, by its base pointer, by a per-channel vector
    T.append(Case("scalar_c8_ld9", "scalar", 8, dense(*row_edges("scalar", 8)), ld=9))
    T.append(Case("scalar_c8_base", "scalar", 8, dense(*row_edges("scalar", 8)), misalign="base"))
    T.append(Case("scalar_c8_vectors", "scalar", 8, dense(*row_edges("scalar", 8)), misalign="vectors"))
    # grids: 1025 tiles on 1024 workgroups, and the bn_tile steps to 32 and 256 rows
    T.append(Case("vec_grid_16385x4", "vec", 4, dense(16385)))
    T.append(Case("scalar_grid_16385x3", "scalar", 3, dense(16385)))
    T.append(Case("vec_grid_65537x8", "vec", 8, dense(65537)))
    T.append(Case("vec_grid_524289x4", "vec", 4, dense(524289)))
    # layouts: ld > C, batch-strided, both
    T.append(Case("vec_wide", "vec", 8, dense(1, 129, 257), ld=24))
    T.append(Case("vec_strided", "vec", 8, (STRIDED, Edge(2, 129, 131), Edge(5, 16, 17))))
    T.append(Case("vec_wide_strided", "vec", 128, (STRIDED, Edge(2, 9, 10), Edge(4, 4, 7)), ld=132))
    T.append(Case("scalar_wide", "scalar", 10, dense(1, 26, 51), ld=13))
    T.append(Case("scalar_strided", "scalar", 10, (STRIDED, Edge(2, 26, 27), Edge(5, 16, 17))))
    T.append(Case("scalar_wide_strided", "scalar", 300, (STRIDED, Edge(2, 9, 10), Edge(4, 4, 7)), ld=301))
    for C in (4, 8, 12, 24, 36, 64, 1024):
        T.append(Case(f"small_c{C}", "small", C, dense(*SMALL_ROWS)))
    T.append(Case("small_wide", "small", 8, dense(1, 1024, 1025), ld=24))
    T.append(Case("small_strided", "small", 12, (STRIDED, Edge(2, 512, 513), Edge(3, 682, 700)), ld=16))
    for C in (4, 32, 256, 1024):
        T.append(Case(f"resid_sweep_c{C}", "resid_sweep", C, dense(*(row_edges("vec", C) + (2049,)))))
        T.append(Case(f"resid_small_c{C}", "resid_small", C, dense(*SMALL_ROWS)))
    T.append(Case("resid_grid_16385x4", "resid_sweep", 4, dense(16385)))
    return T


CASES = _table()
assert len({c.id for c in CASES}) == len(CASES)


@dataclass(frozen=True)
class Opts:
    act: int                 # 0 none / 1 ReLU / 2 LeakyReLU 0.2
    affine: bool             # False: scale = shift = NULL
    items: int               # the batched finalize carries 1, 2 or 8 items
    count3: bool             # (one launch) count = 3 x rows with coef_out requested
    resid_slope: float       # (junction) 0.01 / 0


def options(i: int, j: int) -> Opts:
    """Rotated over (row, edge): 7 i + j walks every residue of 3, 4 and 2 within any family."""
    h = 7 * i + j
    return Opts(act=h % 3, affine=h % 4 != 3, items=(1, 2, 8)[(h // 3) % 3], count3=(h // 2) % 2 == 1, resid_slope=(0.01, 0.0)[h % 2])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Bwd:
    case: Case
    edge: Edge
    opts: Opts
    count: int
    a: dict = field(default_factory=dict)      # numpy arrays by name; G / Y / O / Y1 / Y2 are storage (B * bstride, ld), NaN outside

    @property
    def M(self):
        return self.edge.M

    @property
    def resid(self):
        return self.case.family.startswith("resid")

    def rows(self):
        """Storage row of every logical row."""
        e = self.edge
        return (np.arange(e.B)[:, None] * e.bstride + np.arange(e.n)[None, :]).reshape(-1)

    def logical(self, name):
        return self.a[name][self.rows(), :self.case.C]


def _store(case, e, x):
    s = np.full((e.B * e.bstride, case.lda), np.nan, dtype=F32)
    s.reshape(e.B, e.bstride, case.lda)[:, :e.n, :case.C] = x.reshape(e.B, e.n, case.C)
    return s


def sign_margin(y, sc, sh):
    """Elements whose activation sign an fp32 z could get wrong: |y.sc + sh| < 2^-18 (|y.sc| + |sh|), in fp64."""
    ys = y.astype(F64) * sc.astype(F64)
    return np.abs(ys + sh.astype(F64)) < 2.0 ** -18 * (np.abs(ys) + np.abs(sh.astype(F64)))


def _bn_vectors(rng, Y, C):
    mean = Y.mean(0, dtype=F64).astype(F32) if Y.shape[0] > 1 else (Y[0] - F32(0.25)).astype(F32)
    var = Y.var(0, dtype=F64) if Y.shape[0] > 1 else np.full(C, 0.5)
    invstd = (1.0 / np.sqrt(var + 1e-2)).astype(F32)
    gamma = (rng.random(C) + 0.5).astype(F32)
    beta = (rng.standard_normal(C) * 0.2).astype(F32)
    scale = (gamma * invstd).astype(F32)
    return mean, invstd, scale, (beta - mean * scale).astype(F32)


def make_bwd(case: Case, i: int, j: int) -> Bwd:
    e, o, C = case.edges[j], options(i, j), case.C
    M = e.M
    rng = np.random.default_rng(100000 + 1000 * i + j)
    inp = Bwd(case, e, o, 3 * M if (case.family == "small" and o.count3) else M)
    a = inp.a
    mu, sd = rng.standard_normal(C) * 0.5, rng.random(C) + 0.5
    if inp.resid:
        for k in ("1", "2"):
            Y = (rng.standard_normal((M, C)) * sd + mu).astype(F32)
            a["mean" + k], a["invstd" + k], a["scale" + k], _ = _bn_vectors(rng, Y, C)
            a["Y" + k] = _store(case, e, Y)
        O = rng.standard_normal((M, C)).astype(F32)
        zero = rng.random((M, C))
        O[zero < 0.1] = 0.0                       # O > 0 is false at +0 and at -0: both take the slope
        O[zero < 0.05] = -0.0
        O.reshape(-1)[:2] = (0.0, -0.0)
        a["O"] = _store(case, e, O)
        a["G"] = _store(case, e, rng.standard_normal((M, C)).astype(F32))
        return inp
    Y = (rng.standard_normal((M, C)) * sd + mu).astype(F32)
    a["mean"], a["invstd"], scale, shift = _bn_vectors(rng, Y, C)
    if o.affine:
        a["scale"], a["shift"] = scale, shift
        for _ in range(4):
            bad = sign_margin(Y, scale, shift)
            if not bad.any():
                break
            Y[bad] += F32(0.5)
    else:
        Y[Y == 0] = F32(0.5)
    a["Y"] = _store(case, e, Y)
    a["G"] = _store(case, e, rng.standard_normal((M, C)).astype(F32))
    assert_signs(inp)
    return inp


def assert_signs(inp: Bwd):
    """No element of the row is left whose activation derivative depends on how z was rounded."""
    if inp.resid:
        return
    y = inp.logical("Y")
    if "scale" in inp.a:
        assert not sign_margin(y, inp.a["scale"], inp.a["shift"]).any(), inp.case.id
    else:
        assert not (y == 0).any(), inp.case.id


def act_neg(act: int) -> float:
    return {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU: SLOPE}[act]


# ---- fp64 reference and bounds of the backward ----------------------------------------------------------------------------------------------
def reference_bwd(inp: Bwd) -> dict:
    """Every output in fp64 with its bound: name -> (ref, bound)."""
    C, M, fam = inp.case.C, inp.M, inp.case.family
    D = sum_depth(fam, C, M)
    out = {}

    def sums(term, name):
        ref, env = term.sum(0), np.abs(term).sum(0)
        first = 2 * (D + 4) * U * env
        out[name] = (ref, first + U * np.abs(ref))
        k = ref / inp.count
        return k, first / inp.count + U * np.abs(k)

    def dy(sc, g, k0, dk0, xh, k1, dk1):
        E = np.abs(g) + np.abs(k0) + np.abs(xh * k1)
        return sc * (g - k0 - xh * k1), np.abs(sc) * (M2 * 7 * U * E + dk0 + np.abs(xh) * dk1)

    G = inp.logical("G").astype(F64)
    if inp.resid:
        o = inp.logical("O")
        g = np.where(o > 0, G, G * F64(F32(inp.opts.resid_slope)))
        k0, dk0 = sums(g, "dbeta")
        for k in ("1", "2"):
            xh = (inp.logical("Y" + k).astype(F64) - inp.a["mean" + k].astype(F64)) * inp.a["invstd" + k].astype(F64)
            k1, dk1 = sums(g * xh, "dgamma" + k)
            out["coef" + k] = (np.concatenate([k0, k1]), np.concatenate([dk0, dk1]))
            out["dY" + k] = dy(inp.a["scale" + k].astype(F64), g, k0, dk0, xh, k1, dk1)
        return out
    y = inp.logical("Y").astype(F64)
    sc = inp.a["scale"].astype(F64) if "scale" in inp.a else np.ones(C)
    sh = inp.a["shift"].astype(F64) if "shift" in inp.a else np.zeros(C)
    g = G * np.where(y * sc + sh > 0, 1.0, F64(F32(act_neg(inp.opts.act))))
    xh = (y - inp.a["mean"].astype(F64)) * inp.a["invstd"].astype(F64)
    k0, dk0 = sums(g, "dbeta")
    k1, dk1 = sums(g * xh, "dgamma")
    out["coef"] = (np.concatenate([k0, k1]), np.concatenate([dk0, dk1]))
    out["dY"] = dy(sc, g, k0, dk0, xh, k1, dk1)
    out["dY_act"] = (sc * g, M2 * 2 * U * np.abs(sc * g))         # the apply without coefficients
    return out


def check(got, ref, bound, what=""):
    """The per-element bound; returns max error / bound and asserts it is <= 1 (0 / 0 counts as 0)."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values in the result"
    err = np.abs(got.astype(np.longdouble) - ref).astype(F64)
    ratio = err / np.maximum(np.asarray(bound, dtype=F64), 1e-300)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{what}: element {tuple(int(x) for x in at)} is off by {float(err[at]):.3e}, {worst:.2f} x its bound "
                             f"{float(np.asarray(bound)[at]):.3e} (got {float(got[at])!r}, reference {float(ref[at])!r}); "
                             f"{int((ratio > 1).sum())} of {ratio.size} elements exceed theirs")
    return worst


def silent(before: np.ndarray, after: np.ndarray, inp: Bwd) -> bool:
    """Everything of a storage array outside the addressed block holds its bits."""
    mask = np.ones(before.shape, dtype=bool)
    mask[inp.rows()[:, None], np.arange(inp.case.C)[None, :]] = False
    return np.array_equal(before.view(np.int32)[mask], after.view(np.int32)[mask])


def verify_bwd(inp: Bwd, got: dict, ref: Optional[dict] = None) -> dict:
    """A launch's outputs (the device's or the emulation's) against reference_bwd: name -> error / bound.  `got` holds the storage
    arrays after the launch ("G", "G2", "G_act") and the vectors ("dbeta", "dgamma", "coef", with 1 / 2 at the junction)."""
    ref = ref or reference_bwd(inp)
    where = f"{inp.case.id} {inp.edge}"
    rows, C = inp.rows(), inp.case.C
    ratios = {}
    names = {"G": "dY1", "G2": "dY2"} if inp.resid else {"G": "dY", "G_act": "dY_act"}
    for key, name in names.items():
        if key in got:
            assert silent(inp.a["G"], got[key], inp) or key == "G2", f"{where}: {key} changed outside the addressed block"
            ratios[name] = check(got[key][rows, :C], *ref[name], f"{where} {name}")
    for name in ("dbeta", "dgamma", "coef", "dbeta1", "dbeta2", "dgamma1", "dgamma2", "coef1", "coef2"):
        if name in got:
            r = ref["dbeta"] if name.startswith("dbeta") else ref[name]
            ratios[name] = check(got[name], *r, f"{where} {name}")
    return ratios


# ---- the emulation: which lane adds which rows in which order (fp32), then double --------------------------------------------------------
MUTANTS_BWD = ("tail_dropped", "no_grid_stride", "bstride_ignored", "relu_as_lrelu", "coef_swapped", "xhat_without_invstd",
               "local_rows_for_count", "last_quad_unowned", "second_channel_pass_skipped")
MUTANTS_FOLD = ("unbiased_factor_missing", "pivot_not_added", "bias_missing_from_running_mean")


def _butterfly(a, axis_len):
    """The xor butterfly over axis 2 of (.., .., axis_len, C): every lane ends with the same fp32 sum."""
    idx = np.arange(axis_len)
    s = axis_len >> 1
    while s >= 1:
        a = a + a[:, :, idx ^ s, :]
        s >>= 1
    return a


def _sweep_sums(terms, family, C, M, mutant):
    """Per-channel totals (double) of each (M, C) fp32 term array as the sweep kernels sum them, and the rows they covered."""
    tpr, rpar = lanes(family, C)
    tile = bn_tile(M)
    ntiles = -(-M // tile)
    grid = min(ntiles, MAX_SLOTS)
    trips = 1 if mutant == "no_grid_stride" else -(-ntiles // grid)
    b, r = np.arange(grid)[:, None], np.arange(rpar)[None, :]
    acc = [np.zeros((grid, rpar, C), dtype=F32) for _ in terms]
    covered = np.zeros(M, dtype=bool)
    for t in range(trips):
        tid = b + t * grid
        rend = np.minimum(M, (tid + 1) * tile)
        for k in range(-(-tile // rpar)):
            R = tid * tile + r + k * rpar
            ok = (R < rend) & (tid < ntiles)
            if mutant == "tail_dropped" and family == "vec" and k % 2 == 0:
                ok &= R + rpar < rend                           # the two-rows-per-trip loop without its odd tail
            Rc = np.minimum(R, M - 1)
            covered[Rc[ok]] = True
            for n_, T in enumerate(terms):
                acc[n_] = acc[n_] + np.where(ok[..., None], T[Rc], F32(0))
    out = []
    for a in acc:
        if family != "scalar" and tpr < 64:
            w = 64 // tpr
            a = _butterfly(a.reshape(grid, 4, w, C), w)[:, :, 0, :]
        out.append(a.astype(F64).sum(1).sum(0))                 # the copies in LDS, then the slots: double
    return out, covered


def _small_sums(terms, C, M, mutant):
    """The one-launch kernels: lane t holds rows t and t + 1024, a wave sum, the 16 wavefronts in double; and the owned channels."""
    R = sm_r(M)
    nq = C >> 2
    owned = np.zeros(C, dtype=bool)
    for q in small_quads(C):
        if q >= 0 and not (mutant == "last_quad_unowned" and q == nq - 1):
            owned[4 * q:4 * q + 4] = True
    out = []
    for T in terms:
        P = np.zeros((R * SM_T, C), dtype=F32)
        P[:M] = T
        P = P.reshape(R, SM_T, C)
        a = P[0] if R == 1 else P[0] + P[1]
        a = _butterfly(a.reshape(1, SM_T // 64, 64, C), 64)[0, :, 0, :]
        out.append(a.astype(F64).sum(0))
    return out, owned


def emulate_bwd(inp: Bwd, mutant: Optional[str] = None) -> dict:
    """The launch sequence of the row's family in numpy fp32, same outputs as the device run; `mutant` breaks one thing."""
    case, e, o, C, M = inp.case, inp.edge, inp.opts, inp.case.C, inp.M
    fam = case.family
    rows = inp.rows()
    if mutant == "bstride_ignored":
        rows = np.arange(M)                                     # row_off without the batch stride
    one = F32(1)
    count = M if mutant == "local_rows_for_count" else inp.count
    G = inp.a["G"][rows, :C]
    if inp.resid:
        slope = F32(o.resid_slope)
        g = np.where(inp.a["O"][rows, :C] > 0, G, G * slope)
        xs = [(inp.a["Y" + k][rows, :C] - inp.a["mean" + k]) * inp.a["invstd" + k] for k in ("1", "2")]
        terms = [g, g * xs[0], g * xs[1]]
        if fam == "resid_small":
            (s, q1, q2), owned = _small_sums(terms, C, M, mutant)
            covered = np.ones(M, dtype=bool)
        else:
            (s, q1, q2), covered = _sweep_sums(terms, fam, C, M, mutant)
            owned = np.ones(C, dtype=bool)
        got = {"G": inp.a["G"].copy(), "G2": np.full_like(inp.a["G"], np.nan)}
        k0 = (s / count).astype(F32)
        for k, q, x, key in (("1", q1, xs[0], "G"), ("2", q2, xs[1], "G2")):
            k1 = (q / count).astype(F32)
            got["dbeta" + k], got["dgamma" + k] = s.astype(F32), q.astype(F32)
            got["coef" + k] = np.concatenate([k0, k1])
            res = (g - k0 - x * k1) * inp.a["scale" + k]
            blk = got[key][rows[covered]]
            blk[:, :C] = np.where(owned[None, :], res[covered], blk[:, :C])
            got[key][rows[covered]] = blk
        return got
    Y = inp.a["Y"][rows, :C]
    sc = inp.a["scale"] if "scale" in inp.a else np.full(C, one)
    sh = inp.a["shift"] if "shift" in inp.a else np.zeros(C, dtype=F32)
    act = ACT_LRELU if (mutant == "relu_as_lrelu" and o.act == ACT_RELU) else o.act
    g = G * np.where(Y * sc + sh > 0, one, F32(act_neg(act)))
    xh = (Y - inp.a["mean"]) * inp.a["invstd"]
    chans = np.ones(C, dtype=bool)
    if mutant == "second_channel_pass_skipped" and fam == "scalar":
        chans[256:] = False
    if fam == "small":
        (s, q), owned = _small_sums([g, g * xh], C, M, mutant)
        covered = np.ones(M, dtype=bool)
    else:
        (s, q), covered = _sweep_sums([g, g * xh], fam, C, M, mutant)
        owned = chans
    got = {"dbeta": np.where(owned, s.astype(F32), F32(7)), "dgamma": np.where(owned, q.astype(F32), F32(7))}
    k0, k1 = (s / count).astype(F32), (q / count).astype(F32)
    got["coef"] = np.where(np.tile(owned, 2), np.concatenate([k0, k1]), F32(7))      # (7: the sentinel a kernel did not overwrite)
    if mutant == "coef_swapped":
        k0, k1 = k1, k0
    xa = (Y - inp.a["mean"]) if mutant == "xhat_without_invstd" else xh

    def scatter(res):
        out = inp.a["G"].copy()
        blk = out[rows[covered]]
        blk[:, :C] = np.where(owned[None, :], res[covered], blk[:, :C])
        out[rows[covered]] = blk
        return out

    got["G"] = scatter((g - k0 - xa * k1) * sc)
    if fam != "small":
        got["G_act"] = scatter(g * sc)
    return got


# ---- the forward fold ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Fold:
    id: str
    nslots: int
    C: int
    count: int = 0                   # 0: 4 x nslots
    training: bool = True
    bias: bool = False               # folded bias
    pivot: Optional[str] = None      # "running" | "vector"
    affine: bool = True              # gamma / beta given
    running: bool = True             # running buffers given (training; eval needs them)
    clamp: bool = False              # channel 0's Q/n - (S/n)^2 is negative by rounding

    @property
    def n(self):
        return self.count or 4 * self.nslots


def _fold_table():
    T = []
    for k, ns in enumerate((1, 255, 256, 257, 1024)):
        for m, C in enumerate((1, 5, 64, 1024)):
            if (k + m) % 2 == 0 or C == 5:
                T.append(Fold(f"plain_s{ns}_c{C}", ns, C))
    T += [Fold("bias_s257_c64", 257, 64, bias=True), Fold("pivot_running_s256_c5", 256, 5, pivot="running"),
          Fold("pivot_running_bias_s255_c64", 255, 64, pivot="running", bias=True), Fold("pivot_vector_s1024_c64", 1024, 64, pivot="vector"),
          Fold("pivot_vector_bias_s257_c1024", 257, 1024, pivot="vector", bias=True),
          Fold("pivot_vector_bias_no_running_s1_c5", 1, 5, pivot="vector", bias=True, running=False),
          Fold("eval_s1_c64", 1, 64, training=False), Fold("eval_bias_s1_c1024", 1, 1024, training=False, bias=True),
          Fold("eval_no_affine_s1_c5", 1, 5, training=False, affine=False),
          Fold("count1_s1_c5", 1, 5, count=1), Fold("count1_bias_s1_c64", 1, 64, count=1, bias=True),
          Fold("clamp_s256_c5", 256, 5, clamp=True), Fold("no_affine_s255_c1", 255, 1, affine=False),
          Fold("no_running_s256_c64", 256, 64, running=False), Fold("no_running_bias_s1024_c1", 1024, 1, running=False, bias=True)]
    return T


FOLDS = _fold_table()
FOLD_BATCHES = (1, 24, 25, 49)
SLOT_CASES = [(ns, C) for ns in (1, 64, 191, 192, 193, 256, 257, 1024) for C in (1, 3, 4, 5, 64)]


def batch_items(count: int):
    """The items of a batched fold: C mixed from 1 to 1024, training and eval, every mode, by rotation."""
    Cs = (1, 1024, 5, 64, 3, 257)
    out = []
    for k in range(count):
        C = Cs[k % len(Cs)] if k % 12 < 6 or count < 25 else (k % 7 + 1)
        training = k % 3 != 1
        pivot = (None, "running", "vector")[(k // 3) % 3] if training else None
        out.append(Fold(f"item{k}", (1, 255, 256, 257, 3)[k % 5] if training else 1, C, training=training, bias=k % 2 == 1,
                        pivot=pivot, affine=k % 5 != 4, running=not training or k % 7 != 6 or pivot == "running"))
    return out


def make_fold(f: Fold, seed: int) -> dict:
    """The fold's arguments (numpy): stats (nslots, 2, C) double, the vectors fp32, nbt int64; absent ones missing."""
    rng = np.random.default_rng(7000 + seed)
    C, ns, n = f.C, f.nslots, f.n
    a = {}
    if f.training:
        r = n / ns
        mu = rng.standard_normal(C) * (0.05 if f.pivot else 1.0)
        sd = rng.random(C) + 0.5
        s = r * (mu + sd * rng.standard_normal((ns, C)) / math.sqrt(max(r, 1.0)))
        q = r * (sd ** 2 * (0.5 + rng.random((ns, C))) + (s / r) ** 2)
        if f.clamp:
            m = 3.0 + np.arange(ns) * 0.0
            s[:, 0] = r * m
            q[:, 0] = r * m * m * (1.0 - 2.0 ** -40)
        a["stats"] = np.stack([s, q], 1).astype(F64)
    if f.affine:
        a["gamma"], a["beta"] = (rng.random(C) + 0.5).astype(F32), (rng.standard_normal(C) * 0.3).astype(F32)
    if f.running:
        a["rmean"], a["rvar"] = rng.standard_normal(C).astype(F32), (rng.random(C) + 0.5).astype(F32)
        a["nbt"] = np.array([3 + seed], dtype=np.int64)
    if f.bias:
        a["bias"] = rng.standard_normal(C).astype(F32)
    if f.pivot == "vector":
        a["pivot"] = rng.standard_normal(C).astype(F32)
    return a


def _fsum_cols(x):
    return np.array([math.fsum(x[:, c]) for c in range(x.shape[1])], dtype=np.longdouble)


def reference_fold(f: Fold, a: dict) -> dict:
    """name -> (ref, bound) for scale, shift, save_mean, save_invstd and, where they are written, rmean, rvar, pivot; "nbt" exact."""
    L = np.longdouble
    C, n = f.C, L(f.n)
    z = np.zeros(C, dtype=L)
    fb = a["bias"].astype(L) if f.bias else z
    g = a["gamma"].astype(L) if f.affine else z + 1
    b = a["beta"].astype(L) if f.affine else z
    rm = a["rmean"].astype(L) if f.running else z
    rv = a["rvar"].astype(L) if f.running else z
    if f.training:
        s, q = a["stats"][:, 0], a["stats"][:, 1]
        S, Q = _fsum_cols(s), _fsum_cols(q)
        dS, dQ = f.nslots * V * np.abs(s).sum(0), f.nslots * V * np.abs(q).sum(0)
        # (the pivot is the fp32 difference the producer subtracted per element: part of the inputs, not of the arithmetic under test)
        piv = ((a["pivot"] if f.pivot == "vector" else a["rmean"]) - (a["bias"] if f.bias else F32(0))).astype(L) if f.pivot else z
        ms = S / n
        dms = dS / n + V * np.abs(ms)
        mean = piv + ms
        raw = Q / n - ms * ms
        var = np.maximum(raw, 0)
        big = Q / n + ms * ms
        dvar = dQ / n + 2 * np.abs(ms) * dms + 3 * V * big
        if f.clamp:
            assert raw[0] < 0
            keep = np.arange(C) != 0
            dvar = np.where(keep, dvar, 0)                      # the clamp channel: var = 0 exactly
        else:
            keep = np.ones(C, dtype=bool)
        assert (big[keep] / var[keep] < 2.0 ** 20).all(), f"{f.id}: a vacuous bound (cancellation factor above 2^20)"
    else:
        mean, var, dms, dvar = rm - fb, rv, z, z
    dmean = dms + V * np.abs(mean)
    eps = L(EPS)
    inv = 1 / np.sqrt(var + eps)
    dinv = inv * (dvar / (var + eps) + 4 * V + U)
    sc = g * inv
    dsc = np.abs(g) * dinv + U * np.abs(sc)
    ms_ = np.abs(mean * sc)
    out = {"scale": (sc, dsc), "save_invstd": (inv, dinv), "save_mean": (mean, dmean + U * np.abs(mean)),
           "shift": (b - mean * sc, np.abs(sc) * (dmean + U * np.abs(mean)) + np.abs(mean) * dsc + U * ms_ + U * (np.abs(b) + ms_))}
    if f.training:
        m, am = L(MOMENTUM), L(F32(1) - MOMENTUM)
        y = mean + fb
        dy = dmean + U * np.abs(mean) + U * np.abs(y)
        if f.pivot == "vector":
            out["pivot"] = (y, dy)
        if f.running:
            out["rmean"] = (am * rm + m * y, m * dy + 2 * U * (np.abs(am * rm) + np.abs(m * y)))
            k = n / (n - 1) if f.n > 1 else L(1)
            unb = var * k
            out["rvar"] = (am * rv + m * unb, m * (dvar * k + (2 * V + U) * unb) + 2 * U * (np.abs(am * rv) + np.abs(m * unb)))
            out["nbt"] = int(a["nbt"][0]) + 1
    elif f.running:
        out["nbt"] = int(a["nbt"][0])
    return {k: ((v[0], np.asarray(v[1] * M2, dtype=F64)) if isinstance(v, tuple) else v) for k, v in out.items()}


def slot_sums_wg(x):
    """slot_sums_wg in double: lane t adds slots t, t + 256, ..; a butterfly per wavefront; the four wavefronts in a fixed order."""
    ns, C = x.shape
    P = np.zeros((-(-ns // 256) * 256, C), dtype=F64)
    P[:ns] = x
    a = np.zeros((256, C), dtype=F64)
    for k in range(P.shape[0] // 256):
        a = a + P[256 * k:256 * (k + 1)]
    w = _butterfly(a.reshape(1, 4, 64, C), 64)[0, :, 0, :]
    return (w[0] + w[1]) + (w[2] + w[3])


def slot_sums_wave(x):
    """slot_sums (rl_bn_reduce_slots): one wavefront, four accumulators while four slots per lane remain, then one."""
    ns, C = x.shape
    a = np.zeros((64, C), dtype=F64)
    for lane in range(64):
        acc = [np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)]
        i = lane
        while i + 192 < ns:
            for k in range(4):
                acc[k] = acc[k] + x[i + 64 * k]
            i += 256
        while i < ns:
            acc[0] = acc[0] + x[i]
            i += 64
        a[lane] = (acc[0] + acc[1]) + (acc[2] + acc[3])
    return _butterfly(a.reshape(1, 1, 64, C), 64)[0, 0, 0]


def emulate_fold(f: Fold, a: dict, mutant: Optional[str] = None) -> dict:
    """bn_finalize_body in numpy: double where the kernel is double, fp32 where it is fp32.  Returns what the kernel writes."""
    C = f.C
    one, zero = F32(1), np.zeros(C, dtype=F32)
    fb = a["bias"] if f.bias else zero
    g = a["gamma"] if f.affine else zero + one
    b = a["beta"] if f.affine else zero
    rm = a["rmean"] if f.running else zero
    rv = a["rvar"] if f.running else zero
    count = F64(f.n)
    if f.training:
        s, q = slot_sums_wg(a["stats"][:, 0]), slot_sums_wg(a["stats"][:, 1])
        pv = a["pivot"] if f.pivot == "vector" else rm
        pivot = (pv - fb).astype(F64) if f.pivot else np.zeros(C)
        ms = s / count
        mean = ms if mutant == "pivot_not_added" else pivot + ms
        var = np.maximum(q / count - ms * ms, 0.0)
    else:
        mean, var = rm.astype(F64) - fb.astype(F64), rv.astype(F64)
    invstd = (1.0 / np.sqrt(var + F64(EPS))).astype(F32)
    sc = g * invstd
    out = {"scale": sc, "shift": b - mean.astype(F32) * sc, "save_mean": mean.astype(F32), "save_invstd": invstd}
    if f.training and f.running:
        unb = var * count / (count - 1.0) if (f.n > 1 and mutant != "unbiased_factor_missing") else var
        y = mean.astype(F32) if mutant == "bias_missing_from_running_mean" else mean.astype(F32) + fb
        out["rmean"] = (one - MOMENTUM) * rm + MOMENTUM * y
        out["rvar"] = (one - MOMENTUM) * rv + MOMENTUM * unb.astype(F32)
        out["nbt"] = int(a["nbt"][0]) + 1
    elif f.running:
        out["nbt"] = int(a["nbt"][0])
    if f.training and f.pivot == "vector":
        out["pivot"] = mean.astype(F32) + fb
    return out


def verify_fold(f: Fold, a: dict, got: dict, ref: Optional[dict] = None) -> dict:
    """A fold's outputs against reference_fold; buffers the kernel must not update (eval, null running buffers) are the caller's
    to compare bit for bit."""
    ref = ref or reference_fold(f, a)
    ratios = {}
    for name, r in ref.items():
        if name == "nbt":
            assert got["nbt"] == r, (f.id, "num_batches_tracked", got["nbt"], r)
        else:
            ratios[name] = check(got[name], *r, f"{f.id} {name}")
    if f.clamp:
        assert got["save_invstd"][0] == F32(1.0 / np.sqrt(F64(EPS))), (f.id, "the negative variance was not clamped to 0")
    return ratios


def stored(ref, d):
    """The bound of a double result within d of `ref` once it is rounded to fp32: d + u (|ref| + d)."""
    return np.asarray(d + U * (np.abs(ref) + d), dtype=F64)


def reference_slots(x):
    """rl_bn_reduce_slots of (nslots, 2, C) double partials: (ref (2, C), bound)."""
    ns, _, C = x.shape
    flat = x.reshape(ns, 2 * C)
    return _fsum_cols(flat).reshape(2, C), (ns * V * np.abs(flat).sum(0)).reshape(2, C)
