"""The gather path's kernels (csrc/rows.hip: rl_copy_rows, rl_copy_rows_pair, rl_scatter_add_rows; csrc/csr.hip: rl_csr_build,
rl_segment_sum_rows) as three tables: one row per kernel instantiation, layout and edge, with the inputs, the fp64 references, the
bounds, the host dispatch restated, and numpy emulations of what the kernels compute.  tests/test_gather_lattice_cpu.py checks the
tables against the restated dispatch, the dispatch against the library's host side, and the checkers against the emulations and
their mutants; tests/test_gather_lattice_gpu.py runs every row on the device.

Conventions.  Inputs are NaN-free, from a seed made of the table's number and the row's position.  u = 2^-24, every bound carries
(1 + 2^-10), none is tuned against a kernel:
  * rl_csr_build: integers.  Per cloud the entries with 0 <= idx < n_dst are kept; entries[:kept] is the stable argsort of their
    destinations (ascending source row inside a destination), offsets = 0, cumulative bincount.  What lies behind entries[kept] is
    unspecified and not compared.
  * rl_segment_sum_rows: a destination with n gatherers, a = 1 when accumulating, S = sum|x| + a |old|:
        |dst - ref| <= (1 + 2^-10) max(n - 1 + a, 0) u S
    (sequential adds from a zero accumulator: the first is exact, every later one rounds at most u times a partial sum of
    magnitude <= S).  The order contract: equal by value to the fp32 sum in ascending entry order, then + old.
  * rl_copy_rows: z = x.sc + sh, v = act(z) (+ old):
        |dst - ref| <= (1 + 2^-10) u (2 |x.sc| + |sh| + [LeakyReLU, z < 0] |z.slope| + a (|v| + |old|))
    (the two roundings of z, the slope product, the accumulate add; the activation is continuous, so no element is left out);
    a plain copy is bitwise.  The expression: equal by value to z = fl(fl(x.sc) + sh), v = max(z, z.e) in fp32 (ReLU of a negative
    is -0 on the 16-byte path and +0 on the scalar path: by value, not by bit).
  * rl_scatter_add_rows: a destination element with n contributions: |dst - ref| <= (1 + 2^-10) n u sum|x|, in any order.
Every output lives in a buffer larger than what the kernel may write, pre-filled with the bit pattern SENT; "silence" = every word
outside the addressed block still holds SENT, compared as int32.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

U = 2.0 ** -24
M2 = 1.0 + 2.0 ** -10
F32, F64, I32 = np.float32, np.float64, np.int32
SENT = 0x7FC5A5A5              # a quiet NaN as fp32: anything accumulated onto it shows
GUARD = 64                     # words (256 bytes) of SENT on both sides of every output and of the CSR workspace
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
DROPS = (-1, None, INT32_MAX, INT32_MIN)      # None stands for n_dst
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
SLOPE = 0.2
BIG_CPU = 1 << 20              # rows with more output elements than this are run on the device only


def seed(table: int, i: int) -> int:
    return 100000 * table + i


def check(got, ref, bound, what=""):
    """The per-element bound; returns max error / bound and asserts it is <= 1 (0 / 0 counts as 0)."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values in the result"
    err = np.abs(got.astype(F64) - ref)
    ratio = err / np.maximum(np.asarray(bound, dtype=F64), 1e-300)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{what}: element {tuple(int(x) for x in at)} is off by {float(err[at]):.3e}, {worst:.3g} x its bound "
                             f"{float(np.asarray(bound)[at]):.3e} (got {float(got[at])!r}, reference {float(ref[at])!r}); "
                             f"{int((ratio > 1).sum())} of {ratio.size} elements exceed theirs")
    return worst


def guarded(n: int, dtype=I32) -> np.ndarray:
    """GUARD words, n words, GUARD words, all SENT."""
    return np.full(GUARD + n + GUARD, SENT, dtype=I32).view(dtype)


def silent(buf: np.ndarray, written: Optional[np.ndarray] = None) -> bool:
    """Both guard bands, and every word of the body that `written` (a mask over the body) does not name, hold SENT."""
    w = buf.view(I32)
    body = w[GUARD:len(w) - GUARD]
    ok = bool((w[:GUARD] == SENT).all() and (w[len(w) - GUARD:] == SENT).all())
    if written is not None:
        ok = ok and bool((body[~written.reshape(-1)] == SENT).all())
    return ok


# ==================================================================================================================== graphs
@dataclass(frozen=True)
class Graph:
    """idx (B, n_src, k) with destinations in [0, n_dst).  kind: "uniform"; "near" (row i gathers around i); "degrees" (deg[j]
    gatherers of destination j, positions shuffled; entries left over are dropped indices); "cover" (column 0 a permutation -
    every destination is gathered at least once - the rest uniform); "perm" (k = 1: a permutation with an eighth of the entries
    redirected: duplicates and empty destinations).  dropped: a tenth of the entries become -1, n_dst, INT32_MAX, INT32_MIN."""
    n_src: int
    k: int
    n_dst: int
    kind: str = "uniform"
    deg: Tuple[int, ...] = ()
    dropped: bool = False

    @property
    def per(self) -> int:
        return self.n_src * self.k


def _drop_values(n: int, n_dst: int) -> np.ndarray:
    vals = np.array([n_dst if v is None else v for v in DROPS], dtype=np.int64)
    return vals[np.arange(n) % 4]


def make_idx(g: Graph, B: int, rng) -> np.ndarray:
    out = np.empty((B, g.per), dtype=np.int64)
    for b in range(B):
        if g.kind == "uniform":
            flat = rng.integers(0, g.n_dst, g.per)
        elif g.kind == "near":
            flat = ((np.arange(g.per) // g.k + rng.integers(-40, 41, g.per)) % g.n_dst)
        elif g.kind == "degrees":
            assert len(g.deg) <= g.n_dst and sum(g.deg) <= g.per
            flat = np.repeat(np.arange(len(g.deg)), g.deg)
            rest = g.per - len(flat)
            assert rest == 0 or g.dropped, "a degrees graph with entries left over must be a dropped one"
            flat = rng.permutation(np.concatenate([flat, _drop_values(rest, g.n_dst)]))
        elif g.kind == "cover":
            assert g.n_src == g.n_dst and g.k > 1
            flat = rng.integers(0, g.n_dst, (g.n_src, g.k))
            flat[:, 0] = rng.permutation(g.n_dst)
            flat = flat.reshape(-1)
        elif g.kind == "perm":
            assert g.k == 1 and g.n_src == g.n_dst
            flat = rng.permutation(g.n_dst)
            hit = rng.choice(g.per, g.per // 8, replace=False)
            flat[hit] = rng.integers(0, g.n_dst, len(hit))
        else:
            raise ValueError(g.kind)
        if g.dropped and g.kind != "degrees":
            hit = rng.choice(g.per, max(g.per // 10, min(4, g.per)), replace=False)
            flat = flat.copy()
            flat[hit] = _drop_values(len(hit), g.n_dst)
        out[b] = flat
    return out.astype(I32).reshape(B, g.n_src, g.k)


def csr_reference(idx: np.ndarray, n_dst: int):
    """offsets (B, n_dst + 1), entries (B, per) with -1 behind the kept ones, kept (B,)."""
    B = idx.shape[0]
    flat = idx.reshape(B, -1).astype(np.int64)
    off = np.zeros((B, n_dst + 1), dtype=I32)
    ent = np.full(flat.shape, -1, dtype=I32)
    kept = np.zeros(B, dtype=np.int64)
    for b in range(B):
        pos = np.nonzero((flat[b] >= 0) & (flat[b] < n_dst))[0]
        d = flat[b][pos]
        ent[b, :len(pos)] = pos[np.argsort(d, kind="stable")]
        off[b, 1:] = np.cumsum(np.bincount(d, minlength=n_dst))
        kept[b] = len(pos)
    return off, ent, kept


# ==================================================================================================================== table 1
CSR_MAX_TASKS, CSR_TILE, CSR_BUCKET, CSR_MAX_BUCKETS, LONG_WGS, LONG_CHUNK = 8, 4096, 256, 1024, 128, 1024


def up256(x: int) -> int:
    return (x + 255) & ~255


def two_level_ok(g: Graph) -> bool:
    return -(-g.n_dst // CSR_BUCKET) <= CSR_MAX_BUCKETS and g.per < (1 << 24)


def csr_plan(B: int, tasks) -> dict:
    """csr.hip's make_plan / rl_csr_build restated: per task cap, long_cap, nbuckets, ntiles, bytes; for the call two_level, need[],
    deal (csr_deal on), the grids' x extents and the workspace bytes."""
    two = all(two_level_ok(g) for g in tasks)
    per_task, need = [], [False, False, False]
    for g in tasks:
        mean = float(g.per) / float(g.n_dst)
        if two:
            cap = 32 if mean * 2 <= 32 else 56
        else:
            cap = 32 if mean * 2 <= 32 else (64 if mean * 2 <= 64 else 128)
        ent = B * g.per
        long_cap = ent // cap + 1
        nb, nt = -(-g.n_dst // CSR_BUCKET), -(-g.per // CSR_TILE)
        nbytes = (up256(ent * 4) + (0 if two else up256(B * g.n_dst * 4)) + up256(long_cap * 4) + 256 + up256(B * nb * 4) +
                  up256(B * (nb + 1) * 4))
        need[0 if cap == 32 else (1 if cap in (56, 64) else 2)] = True
        per_task.append(dict(cap=cap, long_cap=long_cap, nbuckets=nb, ntiles=nt, bytes=nbytes))
    return dict(two_level=two, need=need, deal=B > 1 and 8 % B == 0, tasks=per_task, bytes=sum(t["bytes"] for t in per_task),
                max_tiles=max(t["ntiles"] for t in per_task), max_buckets=max(t["nbuckets"] for t in per_task),
                last_kernel="csr2_bucket_kernel" if two else "csr_sort_kernel")


@dataclass(frozen=True)
class CsrRow:
    id: str
    B: int
    tasks: Tuple[Graph, ...]


def _deg(*pairs) -> Tuple[int, ...]:
    """(length, count) pairs -> a degree tuple."""
    out = []
    for length, count in pairs:
        out += [length] * count
    return tuple(out)


def _atomics_task(cap: int, n_dst: int, fill: int) -> Graph:
    """Segments of 0, 1, cap, cap + 1 and 1500 entries, n_dst - 5 of `fill`, a tenth of the cloud dropped."""
    deg = _deg((0, 1), (1, 1), (cap, 1), (cap + 1, 1), (1500, 1), (fill, n_dst - 5))
    kept = sum(deg)
    return Graph(kept + kept // 10, 1, n_dst, "degrees", deg, True)


FORCING = Graph(8, 1, 262145)          # beyond the bucket packing: every task beside it takes the per-entry-atomics path


def _csr_table():
    rows = []
    # bucket borders x tile borders, one row per n_dst with the five entry counts as its tasks; B walks over deal on / off
    for n_dst, B in zip((1, 255, 256, 257, 513), (1, 2, 4, 8, 3)):
        rows.append(CsrRow(f"borders-ndst{n_dst}-B{B}", B, tuple(Graph(e, 1, n_dst) for e in (1, 4095, 4096, 4097, 8193))))
    for B in (1, 2, 4, 8, 3, 5):
        rows.append(CsrRow(f"uniform-B{B}", B, (Graph(700, 16, 700),)))
    rows.append(CsrRow("near-B2", 2, (Graph(3000, 16, 3000, "near"),)))
    rows.append(CsrRow("mean16-cap32", 2, (Graph(600, 16, 600),)))
    rows.append(CsrRow("mean16+-cap56", 2, (Graph(601, 16, 600),)))
    rows.append(CsrRow("len32-33-cap32", 2, (Graph(1261, 1, 300, "degrees", _deg((32, 1), (33, 1), (0, 2), (1, 96), (2, 100), (9, 100))),)))
    rows.append(CsrRow("len56-57-cap56", 2, (Graph(6033, 1, 300, "degrees", _deg((56, 1), (57, 1), (0, 2), (20, 296))),)))
    rows.append(CsrRow("one-destination", 2, tuple(Graph(n, 1, 300, "degrees", _deg((0, 7), (n, 1))) for n in (1024, 1025, 2049))))
    rows.append(CsrRow("300-long-segments", 1, (Graph(1125, 16, 300, "degrees", _deg((60, 300))),)))
    rows.append(CsrRow("dropped", 2, (Graph(1000, 16, 1000, dropped=True),)))
    engine = [Graph(n, 16, n, "near") for n in (1024, 256, 64, 16)] + [Graph(n, 1, n // 4) for n in (1024, 256, 64)]
    rows.append(CsrRow("eight-tasks", 4, tuple(engine + [Graph(100, 16, 90)])))
    rows.append(CsrRow("nine-graphs", 2, tuple(engine + [Graph(100, 16, 90), Graph(50, 3, 40, dropped=True)])))
    for B in (1, 2):
        rows.append(CsrRow(f"atomics-B{B}", B, (FORCING, _atomics_task(32, 400, 4), _atomics_task(64, 200, 14), _atomics_task(128, 100, 30))))
    return rows


CSR_ROWS = _csr_table()


def csr_chunks(row: CsrRow):
    """The calls a row makes: at most CSR_MAX_TASKS tasks each (as ops.csr_build splits them)."""
    return [row.tasks[c:c + CSR_MAX_TASKS] for c in range(0, len(row.tasks), CSR_MAX_TASKS)]


def make_csr(i: int):
    """[(graph, idx, ref offsets, ref entries, kept)] of row i."""
    row = CSR_ROWS[i]
    rng = np.random.default_rng(seed(1, i))
    out = []
    for g in row.tasks:
        idx = make_idx(g, row.B, rng)
        out.append((g, idx) + csr_reference(idx, g.n_dst))
    return out


def csr_reached(B: int, tasks, data) -> set:
    """The kernels (and the parts of them) one call reaches, from the restated plan and the segment lengths of its data."""
    plan = csr_plan(B, tasks)
    r = set()
    for (g, idx, off, ent, kept), t in zip(data, plan["tasks"]):
        lens = np.diff(off.astype(np.int64), axis=1)
        nlong = int((lens > t["cap"]).sum())
        pre = "csr2" if plan["two_level"] else "csr"
        r.add(f"csr2_bucket_kernel<{t['cap']}>" if plan["two_level"] else f"csr_sort_kernel<{t['cap']}>")
        if nlong:
            r.add(f"{pre}_sort_long_kernel")
        if nlong > LONG_WGS:
            r.add(f"{pre}_sort_long_kernel:grid-stride")
        if int(lens.max()) > LONG_CHUNK and nlong:
            r.add(f"{pre}_sort_long_kernel:second-chunk")
        if (lens == 1).any() and not plan["two_level"]:
            r.add("csr_sort_kernel:len1")
        if t["ntiles"] < plan["max_tiles"]:
            r.add("early-return:tiles")
        if t["nbuckets"] < plan["max_buckets"]:
            r.add("early-return:buckets")
        if (kept < g.per).any():
            r.add("dropped")
    if plan["two_level"] and plan["need"][0] and plan["need"][1]:
        r.add("both-bucket-kernels")
    if plan["deal"]:
        r.add(f"deal-B{B}")
    return r


def verify_csr(g: Graph, off_ref, ent_ref, kept, off_buf, ent_buf, what=""):
    """Guarded offsets / entries buffers against the reference: integer equality, silence around."""
    B = off_ref.shape[0]
    off = off_buf.view(I32)[GUARD:-GUARD].reshape(B, g.n_dst + 1)
    ent = ent_buf.view(I32)[GUARD:-GUARD].reshape(B, g.per)
    assert silent(off_buf) and silent(ent_buf), f"{what}: wrote outside offsets / entries"
    if not np.array_equal(off, off_ref):
        b, j = np.argwhere(off != off_ref)[0]
        raise AssertionError(f"{what}: offsets[{b}][{j}] = {off[b, j]}, reference {off_ref[b, j]}")
    for b in range(B):
        n = int(kept[b])
        assert n == off_ref[b, -1]
        if not np.array_equal(ent[b, :n], ent_ref[b, :n]):
            e = int(np.argwhere(ent[b, :n] != ent_ref[b, :n])[0, 0])
            raise AssertionError(f"{what}: entries[{b}][{e}] = {ent[b, e]}, reference {ent_ref[b, e]} (of {n} kept)")


CSR_MUTANTS = ("kept_a_dropped_entry", "offsets_shifted", "arrival_order")


def emulate_csr(g: Graph, idx: np.ndarray, mutant: Optional[str] = None):
    """A counting sort as the kernels do it (count, scan, place, sort each segment) -> guarded (offsets, entries)."""
    B = idx.shape[0]
    flat = idx.reshape(B, -1).astype(np.int64)
    off_buf, ent_buf = guarded(B * (g.n_dst + 1)), guarded(B * g.per)
    off = off_buf[GUARD:-GUARD].reshape(B, g.n_dst + 1)
    ent = ent_buf[GUARD:-GUARD].reshape(B, g.per)
    rng = np.random.default_rng(7)
    for b in range(B):
        if mutant == "kept_a_dropped_entry":
            keep = (flat[b] >= 0) & (flat[b] <= g.n_dst)          # <= : n_dst itself slips through, counted with the last destination
        else:
            keep = flat[b].astype(np.uint32) < np.uint32(g.n_dst)  # the kernels' one unsigned compare
        pos = np.nonzero(keep)[0]
        d = np.minimum(flat[b][pos], g.n_dst - 1)
        counts = np.zeros(g.n_dst, dtype=np.int64)
        np.add.at(counts, d, 1)
        start = np.concatenate([[0], np.cumsum(counts)])
        arrival = rng.permutation(len(pos))                          # the order entries arrive in never matters
        order = arrival[np.argsort(d[arrival], kind="stable")]       # placed by destination, arrival order inside
        placed = pos[order]
        if mutant != "arrival_order":
            seg = np.repeat(np.arange(g.n_dst), counts)
            placed = placed[np.lexsort((placed, seg))]               # every segment sorted by rank
        ent[b, :len(pos)] = placed
        off[b] = start + (1 if mutant == "offsets_shifted" else 0)
    return off_buf, ent_buf


# ==================================================================================================================== table 2
def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(F32)


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """The int16 words of values that are already bf16-representable."""
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


@dataclass(frozen=True)
class SegRow:
    id: str
    C: int
    B: int
    g: Graph
    bf16: bool = False
    col0: int = 0          # the source's column offset inside its wider rows
    lds_pad: int = 0       # lds = col0 + C + lds_pad
    sbs_pad: int = 0       # src_bstride = per + sbs_pad
    dbs_pad: int = 0       # dst_bstride = n_dst + dbs_pad
    ldd_pad: int = 0       # ldd = C + ldd_pad
    acc: bool = False
    chain: bool = False    # the device's own CSR feeds the sum (as the engine does)

    lds = property(lambda s: s.col0 + s.C + s.lds_pad)
    ldd = property(lambda s: s.C + s.ldd_pad)
    src_bstride = property(lambda s: s.g.per + s.sbs_pad)
    dst_bstride = property(lambda s: s.g.n_dst + s.dbs_pad)
    total = property(lambda s: s.B * s.g.n_dst)
    src_rows = property(lambda s: (s.B - 1) * s.src_bstride + s.g.per)
    dst_rows = property(lambda s: (s.B - 1) * s.dst_bstride + s.g.n_dst + 3)     # three rows after the last one
    big = property(lambda s: s.total * s.C > BIG_CPU)


def seg_dispatch(r: SegRow) -> dict:
    """rl_segment_sum_rows' choice restated (both bases sit on 256-byte boundaries; the column offset alone can misalign src)."""
    es = 2 if r.bf16 else 4
    vec = r.C % 4 == 0 and r.lds % 4 == 0 and r.ldd % 4 == 0 and (r.col0 * es) % (8 if r.bf16 else 16) == 0
    if not vec:
        g = min(max(-(-r.total * r.C // 256), 1), 8192)
        return dict(kernel="segment_sum_kernel", vec=False, tpr=0, rpw=0, g=g, capped=r.total * r.C > 8192 * 256, chunk=0, refused=r.bf16)
    tpr = 1
    while tpr < r.C // 4 and tpr < 256:
        tpr <<= 1
    rpw = 256 // tpr
    g_raw = -(-r.total // rpw)
    g = min(max(g_raw, 1), 8192)
    chunk = -(-r.total // 8) if (r.C <= 16 and g >= 8 and g % 8 == 0) else 0
    return dict(kernel="segment_sum_vec_kernel", vec=True, tpr=tpr, rpw=rpw, g=g, capped=g_raw > 8192, chunk=chunk, refused=False,
                column_trips=-(-r.C // (tpr * 4)), in_chunk_trips=-(-chunk // ((g // 8) * rpw)) if chunk else 0)


DEG_SET = (0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 15, 16, 17, 23, 24, 25, 40)
G_SMALL = Graph(150, 4, 130)
G_DEG = Graph(111, 2, 20, "degrees", DEG_SET)           # sum(DEG_SET) = 222; two more destinations stay empty
VEC_C = ((4, 1), (8, 2), (12, 4), (16, 4), (20, 8), (32, 8), (64, 16), (128, 32), (256, 64), (512, 128), (1024, 256), (1028, 256),
         (2048, 256))
XCD_ROWS = ((4, 1, 2041, 8), (8, 3, 299, 8), (12, 3, 169, 8), (16, 3, 169, 8), (16, 1, 1021, 16))    # C, B, n_dst, g


def _seg_table():
    rows = []
    for n, (C, _) in enumerate(VEC_C):
        rows.append(SegRow(f"vec-C{C}", C, 2, G_SMALL, acc=bool(n % 2)))
    for n, C in enumerate((1, 3, 10)):
        rows.append(SegRow(f"scalar-C{C}", C, 2, G_SMALL, acc=bool(n % 2)))
    rows.append(SegRow("scalar-C8-lds10", 8, 2, G_SMALL, lds_pad=2))
    rows.append(SegRow("scalar-C8-col2", 8, 2, G_SMALL, col0=2, lds_pad=2, acc=True))
    for n, C in enumerate((4, 8, 16, 32, 64, 256, 512, 1024)):
        rows.append(SegRow(f"bf16-C{C}", C, 2, G_SMALL, bf16=True, acc=bool(n % 2)))
    rows.append(SegRow("bf16-C16-col4", 16, 2, G_SMALL, bf16=True, col0=4, lds_pad=4))
    rows.append(SegRow("bf16-C128-col4", 128, 2, G_SMALL, bf16=True, col0=4, lds_pad=4, acc=True))
    rows.append(SegRow("bf16-C2048", 2048, 1, Graph(40, 4, 30), bf16=True))
    for C in (4, 16, 64, 1024):
        for bf in (False, True):
            rows.append(SegRow(f"degrees-C{C}-{'bf16' if bf else 'fp32'}", C, 2, G_DEG, bf16=bf, acc=(C == 16)))
    for C, B, n_dst, _ in XCD_ROWS:
        rows.append(SegRow(f"xcd-C{C}-B{B}-n{n_dst}", C, B, Graph(n_dst, 5, n_dst, "cover"), acc=(B == 3 and C == 16)))
    rows.append(SegRow("xcd-C16-B1-n1021-bf16", 16, 1, Graph(1021, 5, 1021, "cover"), bf16=True))
    rows.append(SegRow("unchunked-C16-total513", 16, 1, Graph(513, 5, 513, "cover")))
    rows.append(SegRow("capped-C16-total524289", 16, 1, Graph(524289, 1, 524289, "perm")))
    rows.append(SegRow("capped-C512-total16385", 512, 1, Graph(16385, 1, 16385, "perm"), acc=True))
    for acc in (False, True):
        a = "-acc" if acc else ""
        rows.append(SegRow(f"stride-src{a}", 8, 3, G_SMALL, sbs_pad=7, acc=acc))
        rows.append(SegRow(f"stride-dst{a}", 64, 3, G_SMALL, dbs_pad=5, acc=acc))
        rows.append(SegRow(f"stride-lds-col{a}", 16, 3, G_SMALL, col0=4, lds_pad=8, acc=acc))
        rows.append(SegRow(f"stride-ldd{a}", 32, 3, G_SMALL, ldd_pad=8, acc=acc))
        rows.append(SegRow(f"stride-ldd-scalar{a}", 3, 3, G_SMALL, ldd_pad=2, dbs_pad=1, acc=acc))
    rows.append(SegRow("chained-device-csr", 32, 2, Graph(500, 16, 500, "near"), chain=True))
    return rows


SEG_ROWS = _seg_table()


@dataclass
class Seg:
    row: SegRow
    idx: np.ndarray
    off: np.ndarray
    ent: np.ndarray
    x: np.ndarray              # (src_rows, lds) fp32 (bf16-representable when row.bf16)
    old: Optional[np.ndarray]  # (B, n_dst, C)


def make_seg(i: int) -> Seg:
    r = SEG_ROWS[i]
    rng = np.random.default_rng(seed(2, i))
    idx = make_idx(r.g, r.B, rng)
    off, ent, _ = csr_reference(idx, r.g.n_dst)
    x = (rng.standard_normal((r.src_rows, r.lds), dtype=F32) * np.exp2(rng.integers(-3, 4, (r.src_rows, 1))).astype(F32)).astype(F32)
    if r.bf16:
        x = bf16_round(x)
    old = rng.standard_normal((r.B, r.g.n_dst, r.C), dtype=F32) if r.acc else None
    return Seg(r, idx, off, ent, x, old)


def seg_indices_in_range(s: Seg):
    r = s.row
    o = s.off.astype(np.int64)
    assert (np.diff(o, axis=1) >= 0).all() and (o[:, 0] == 0).all() and (o[:, -1] <= r.g.per).all()
    for b in range(r.B):
        e = s.ent[b, :o[b, -1]]
        assert e.min(initial=0) >= 0 and e.max(initial=0) < r.g.per and b * r.src_bstride + int(e.max(initial=0)) < r.src_rows


def seg_written(r: SegRow) -> np.ndarray:
    m = np.zeros((r.dst_rows, r.ldd), dtype=bool)
    for b in range(r.B):
        m[b * r.dst_bstride: b * r.dst_bstride + r.g.n_dst, :r.C] = True
    return m


def seg_initial(s: Seg) -> np.ndarray:
    """The guarded destination storage before the launch: SENT everywhere, `old` in the addressed block when accumulating."""
    r = s.row
    buf = guarded(r.dst_rows * r.ldd, F32)
    body = buf[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)
    if r.acc:
        for b in range(r.B):
            body[b * r.dst_bstride: b * r.dst_bstride + r.g.n_dst, :r.C] = s.old[b]
    return buf


def _seg_reduce(vals: np.ndarray, off: np.ndarray) -> np.ndarray:
    out = np.zeros((len(off) - 1, vals.shape[1]), dtype=vals.dtype)
    nz = off[1:] > off[:-1]
    if nz.any():
        out[nz] = np.add.reduceat(vals[:off[-1]], off[:-1][nz], axis=0)
    return out


def reference_seg(s: Seg):
    """(ref, bound), both (B, n_dst, C) fp64."""
    r = s.row
    ref = np.zeros((r.B, r.g.n_dst, r.C))
    bound = np.zeros_like(ref)
    for b in range(r.B):
        o = s.off[b].astype(np.int64)
        rows = b * r.src_bstride + s.ent[b, :o[-1]].astype(np.int64)
        v = s.x[rows, r.col0:r.col0 + r.C].astype(F64)
        ref[b] = _seg_reduce(v, o)
        S = _seg_reduce(np.abs(v), o)
        n = np.diff(o)[:, None].astype(F64)
        a = 0.0
        if r.acc:
            ref[b] += s.old[b].astype(F64)
            S += np.abs(s.old[b].astype(F64))
            a = 1.0
        bound[b] = M2 * np.maximum(n - 1 + a, 0) * U * S
    return ref, bound


SEG_MUTANTS = ("descending", "last_entry_dropped", "accumulate_dropped", "src_bstride_off_by_one", "first_row_of_chunk_skipped")


def emulate_seg(s: Seg, mutant: Optional[str] = None, off=None, ent=None) -> np.ndarray:
    """The kernel in fp32: a zero accumulator, the segment's rows added in entry order, then + old -> the guarded storage."""
    r = s.row
    off = s.off if off is None else off
    ent = s.ent if ent is None else ent
    buf = seg_initial(s)
    body = buf[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)
    sbs = r.src_bstride + (1 if mutant == "src_bstride_off_by_one" else 0)
    d = seg_dispatch(r)
    chunk = d["chunk"] if d["vec"] else 0
    for b in range(r.B):
        o = off[b].astype(np.int64)
        lens = np.diff(o)
        if mutant == "last_entry_dropped":
            lens = np.maximum(lens - (lens > 1), 0)
        acc = np.zeros((r.g.n_dst, r.C), dtype=F32)
        for t in range(int(lens.max(initial=0))):
            live = np.nonzero(lens > t)[0]
            e = o[live] + (lens[live] - 1 - t if mutant == "descending" else t)
            rows = np.minimum(b * sbs + ent[b, e].astype(np.int64), s.x.shape[0] - 1)
            acc[live] = acc[live] + s.x[rows, r.col0:r.col0 + r.C]
        if r.acc and mutant != "accumulate_dropped":
            acc = acc + s.old[b]
        lo = b * r.dst_bstride
        if mutant == "first_row_of_chunk_skipped" and chunk:
            keep = (b * r.g.n_dst + np.arange(r.g.n_dst)) % chunk != 0
            body[lo:lo + r.g.n_dst, :r.C][keep] = acc[keep]
        else:
            body[lo:lo + r.g.n_dst, :r.C] = acc
    return buf


def verify_seg(s: Seg, after: np.ndarray, ref=None, emu=None, what="") -> float:
    """The guarded storage after the launch: silence, the fp64 bound per element, the order contract by value.  Returns error / bound."""
    r = s.row
    what = what or r.id
    assert silent(after, seg_written(r)), f"{what}: wrote outside the addressed block"
    ref, bound = ref if ref is not None else reference_seg(s)
    body = after[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)
    got = np.stack([body[b * r.dst_bstride: b * r.dst_bstride + r.g.n_dst, :r.C] for b in range(r.B)])
    worst = check(got, ref, bound, what)
    emu = emulate_seg(s) if emu is None else emu
    ebody = emu[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)
    want = np.stack([ebody[b * r.dst_bstride: b * r.dst_bstride + r.g.n_dst, :r.C] for b in range(r.B)])
    if not np.array_equal(got, want):
        b, j, c = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: dst[{b}][{j}][{c}] = {got[b, j, c]!r} is not the sum in segment order {want[b, j, c]!r} "
                             f"({int((got != want).sum())} elements differ)")
    if not r.acc:       # an empty segment writes +0.0
        empty = np.diff(s.off.astype(np.int64), axis=1) == 0
        assert (got.view(I32)[empty] == 0).all(), f"{what}: an empty segment did not write +0.0"
    return worst


# ==================================================================================================================== table 3
INDEX_KINDS = ("none", "i32", "i64", "i32s", "i64s")
LAZY_KINDS = ("none", "id", "relu", "lrelu")
QUAD_C, SCALAR_C = (4, 8, 12, 64, 256), (1, 3, 6, 10)
ROWS_N = (1, 3, 4, 5, 255, 257, 1023, 1031)
WIDE = 1 << 32


@dataclass(frozen=True)
class CopyRow:
    id: str
    C: int
    n: int                 # rows per cloud
    B: int
    index: str = "none"
    lazy: str = "none"
    acc: bool = False
    c0s: int = 0
    lds_pad: int = 0
    c0d: int = 0
    ldd_pad: int = 0
    scale_off: int = 0     # the lazy vectors start this many floats past a 16-byte boundary
    n_src: int = 0         # rows per cloud of the source (the index's range); 0: n
    wide: bool = False     # rows_per_batch = 2^32 (B = 1): the 64-bit instantiations

    rows = property(lambda s: s.B * s.n)
    rows_per_batch = property(lambda s: WIDE if s.wide else s.n)
    lds = property(lambda s: s.c0s + s.C + s.lds_pad)
    ldd = property(lambda s: s.c0d + s.C + s.ldd_pad)
    src_n = property(lambda s: s.n_src or s.n)
    src_bstride = property(lambda s: s.src_n + 3)            # never rows_per_batch
    src_rows = property(lambda s: s.B * s.src_bstride)
    dst_rows = property(lambda s: s.rows + 3)
    big = property(lambda s: s.rows * s.C > BIG_CPU)
    act = property(lambda s: {"none": ACT_NONE, "id": ACT_NONE, "relu": ACT_RELU, "lrelu": ACT_LRELU}[s.lazy])
    eff = property(lambda s: {"none": 1.0, "id": 1.0, "relu": 0.0, "lrelu": SLOPE}[s.lazy])


def fits32(x: int) -> bool:
    return x < (1 << 32)


def grid_for(work: int) -> int:
    return min(max(-(-work // 256), 1), 4096)


def copy_dispatch(r: CopyRow) -> dict:
    """rl_copy_rows' choice restated (bases on 256-byte boundaries: the column offsets and the lazy vectors' offset decide)."""
    v4 = (r.C % 4 == 0 and r.lds % 4 == 0 and r.ldd % 4 == 0 and r.c0s % 4 == 0 and r.c0d % 4 == 0 and
          (r.lazy == "none" or r.scale_off % 4 == 0))
    small = fits32(r.rows * r.C) and fits32(r.rows_per_batch)
    chunks = r.rows * (r.C // 4) if v4 else r.rows * r.C
    work = -(-chunks // 4) if v4 else chunks
    g = grid_for(work)
    per_trip = g * 256 * (4 if v4 else 1)
    return dict(vec=4 if v4 else 1, itype="uint32_t" if small else "int64_t", grid=g, chunks=chunks, per_trip=per_trip,
                trips=-(-chunks // per_trip), kernel=f"copy_rows_kernel<{4 if v4 else 1}, {'uint32_t' if small else 'int64_t'}>")


def pair_eligible(r: CopyRow) -> bool:
    d = copy_dispatch(r)
    return r.rows > 0 and d["vec"] == 4 and d["itype"] == "uint32_t"


def _copy_table():
    rows = []
    q = 0
    for B in (1, 3):
        for rn in ROWS_N:
            for s, (path, Cs) in enumerate((("quad", QUAD_C), ("scalar", SCALAR_C))):
                C = Cs[q % len(Cs)]
                index, lazy, acc = INDEX_KINDS[(q + s) % 5], LAZY_KINDS[(q // 2 + s) % 4], (q + s) % 3 == 0
                rows.append(CopyRow(f"{path}-C{C}-n{rn}-B{B}-{index}-{lazy}{'-acc' if acc else ''}", C, rn, B, index, lazy, acc,
                                    n_src=0 if index == "none" else rn // 2 + 7))
            q += 1
    # every option on both paths at one shape: index kinds x lazy kinds x accumulate
    for path, C in (("quad", 8), ("scalar", 6)):
        for ik, index in enumerate(INDEX_KINDS):
            for lk, lazy in enumerate(LAZY_KINDS):
                acc = bool((ik + lk) % 2)
                rows.append(CopyRow(f"{path}-C{C}-{index}-{lazy}{'-acc' if acc else ''}", C, 257, 3, index, lazy, acc,
                                    n_src=0 if index == "none" else 100))
    rows.append(CopyRow("scalar-C4-col2", 4, 257, 3, "i32", "lrelu", True, c0s=2, lds_pad=2, n_src=90))
    rows.append(CopyRow("scalar-C8-lds10", 8, 257, 3, "i64s", "relu", False, lds_pad=2, n_src=90))
    rows.append(CopyRow("scalar-C8-scale-odd", 8, 257, 3, "i32", "lrelu", True, scale_off=1, n_src=90))
    rows.append(CopyRow("quad-C8-dstcol-ldd", 8, 257, 3, "i32", "relu", True, c0d=4, ldd_pad=4, n_src=90))
    rows.append(CopyRow("quad-C8-dstcol-ldd-copy", 8, 255, 3, c0d=8, ldd_pad=4, c0s=4, lds_pad=4))
    rows.append(CopyRow("scalar-C3-dstcol-ldd", 3, 257, 3, "i64", "lrelu", False, c0d=1, ldd_pad=2, n_src=90))
    rows.append(CopyRow("capped-grid-C64-rows262145", 64, 262145, 1, "i32", "lrelu", True, n_src=1000))
    rows.append(CopyRow("wide-quad-int64", 8, 1000, 1, "i64", "lrelu", True, n_src=300, wide=True))
    rows.append(CopyRow("wide-scalar-int64", 3, 1000, 1, "i32", "relu", False, n_src=300, wide=True))
    return rows


COPY_ROWS = _copy_table()
# the halves of rl_copy_rows_pair: (first, second, the kernel rl_last_kernel names)
PAIR_ROWS = (
    (CopyRow("pair-a-2720x8", 8, 170 * 16, 1), CopyRow("pair-b-1000x32", 32, 1000, 1, "i32", "lrelu", False, n_src=400), "copy_rows_pair_kernel"),
    (CopyRow("pair-a-1000x64-acc", 64, 500, 2, "i64s", "relu", True, n_src=77), CopyRow("pair-b-5x4", 4, 5, 1, c0d=4, ldd_pad=4),
     "copy_rows_pair_kernel"),
    (CopyRow("pair-a-2720x8", 8, 170 * 16, 1), CopyRow("pair-b-1000x6", 6, 1000, 1, "i32", "lrelu", False, n_src=400), "copy_rows_kernel"),
)


@dataclass
class Copy:
    row: CopyRow
    x: np.ndarray                  # (src_rows, lds)
    index: Optional[np.ndarray]    # int64 values; (rows,) or (n,) when shared
    scale: Optional[np.ndarray]
    shift: Optional[np.ndarray]
    old: Optional[np.ndarray]      # (rows, C)


def make_copy(r: CopyRow, sd: int) -> Copy:
    rng = np.random.default_rng(sd)
    x = (rng.standard_normal((r.src_rows, r.lds), dtype=F32) * np.exp2(rng.integers(-3, 4, (r.src_rows, 1))).astype(F32)).astype(F32)
    index = None
    if r.index != "none":
        index = rng.integers(0, r.src_n, r.n if r.index.endswith("s") else r.rows)
    scale = shift = None
    if r.lazy != "none":
        scale = (rng.uniform(0.5, 1.5, r.C) * rng.choice([-1.0, 1.0], r.C)).astype(F32)
        shift = rng.standard_normal(r.C).astype(F32)
    old = rng.standard_normal((r.rows, r.C), dtype=F32) if r.acc else None
    return Copy(r, x, index, scale, shift, old)


def copy_src_rows(c: Copy, bstride_off: int = 0) -> np.ndarray:
    """The source row of every destination row (the ABI's formula), asserted in range."""
    r = c.row
    rr = np.arange(r.rows)
    b, i = rr // r.rows_per_batch, rr % r.rows_per_batch
    j = i if c.index is None else (c.index[i] if r.index.endswith("s") else c.index[rr])
    if c.index is not None:
        assert j.min() >= 0 and j.max() < r.src_n
    rows = b * (r.src_bstride + bstride_off) + j
    assert bstride_off or (rows.min() >= 0 and rows.max() < r.src_rows)
    return np.minimum(rows, r.src_rows - 1)


def copy_written(r: CopyRow) -> np.ndarray:
    m = np.zeros((r.dst_rows, r.ldd), dtype=bool)
    m[:r.rows, r.c0d:r.c0d + r.C] = True
    return m


def copy_initial(c: Copy) -> np.ndarray:
    r = c.row
    buf = guarded(r.dst_rows * r.ldd, F32)
    if r.acc:
        buf[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)[:r.rows, r.c0d:r.c0d + r.C] = c.old
    return buf


def reference_copy(c: Copy):
    r = c.row
    x = c.x[copy_src_rows(c), r.c0s:r.c0s + r.C].astype(F64)
    if r.lazy == "none":
        v, bound = x, np.zeros_like(x)
    else:
        sc, sh = c.scale.astype(F64), c.shift.astype(F64)
        z = x * sc + sh
        v = np.maximum(z, z * F64(F32(r.eff))) if r.lazy != "id" else z
        bound = 2 * np.abs(x * sc) + np.abs(sh)
        if r.lazy == "lrelu":
            bound = bound + np.where(z < 0, np.abs(z * F64(F32(SLOPE))), 0.0)
    if r.acc:
        bound = bound + np.abs(v) + np.abs(c.old.astype(F64))
        v = v + c.old.astype(F64)
    return v, M2 * U * bound


COPY_MUTANTS = ("accumulate_dropped", "src_bstride_off_by_one")


def emulate_copy(c: Copy, mutant: Optional[str] = None) -> np.ndarray:
    r = c.row
    buf = copy_initial(c)
    v = c.x[copy_src_rows(c, 1 if mutant == "src_bstride_off_by_one" else 0), r.c0s:r.c0s + r.C]
    if r.lazy != "none":
        z = (v * c.scale).astype(F32) + c.shift
        v = np.maximum(z, (z * F32(r.eff)).astype(F32))
    if r.acc and mutant != "accumulate_dropped":
        v = v + c.old
    buf[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)[:r.rows, r.c0d:r.c0d + r.C] = v
    return buf


def verify_copy(c: Copy, after: np.ndarray, what="") -> float:
    r = c.row
    what = what or r.id
    assert silent(after, copy_written(r)), f"{what}: wrote outside the addressed block"
    got = after[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)[:r.rows, r.c0d:r.c0d + r.C]
    ref, bound = reference_copy(c)
    worst = check(got, ref, bound, what)
    want = emulate_copy(c)[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)[:r.rows, r.c0d:r.c0d + r.C]
    if r.lazy == "none" and not r.acc:
        assert np.array_equal(got.view(I32), want.view(I32)), f"{what}: a plain copy is not bitwise"
    if not np.array_equal(got, want):
        i, j = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: dst[{i}][{j}] = {got[i, j]!r}, the fp32 expression gives {want[i, j]!r} ({int((got != want).sum())} differ)")
    return worst


# ---- rl_scatter_add_rows
@dataclass(frozen=True)
class ScatRow:
    id: str
    C: int
    n: int                 # source rows per cloud
    B: int
    index: str             # i32 / i64 / i32s / i64s
    n_dst: int             # the index's range
    wide: bool = False
    c0s: int = 4
    ldd_pad: int = 3

    rows = property(lambda s: s.B * s.n)
    rows_per_batch = property(lambda s: WIDE if s.wide else s.n)
    lds = property(lambda s: s.c0s + s.C + 1)
    ldd = property(lambda s: s.C + s.ldd_pad)
    dst_bstride = property(lambda s: s.n_dst + 2)
    dst_rows = property(lambda s: s.B * s.dst_bstride + 1)


SCAT_ROWS = tuple(
    [ScatRow(f"C{C}-{ix}-B{B}", C, 1000, B, ix, 13 if ix.endswith("s") else 300) for C in (1, 8) for ix, B in (("i32", 3), ("i64", 2), ("i32s", 3), ("i64s", 2))] +
    [ScatRow("C8-duplicates", 8, 4000, 2, "i32", 5), ScatRow("C1-duplicates", 1, 4000, 2, "i64", 3),
     ScatRow("wide-int64", 8, 1000, 1, "i32", 40, wide=True)])


def make_scat(i: int):
    r = SCAT_ROWS[i]
    rng = np.random.default_rng(seed(4, i))
    x = rng.standard_normal((r.rows, r.lds), dtype=F32)
    index = rng.integers(0, r.n_dst, r.n if r.index.endswith("s") else r.rows)
    return r, x, index


def scat_dst_rows(r: ScatRow, index) -> np.ndarray:
    rr = np.arange(r.rows)
    b, i = rr // r.rows_per_batch, rr % r.rows_per_batch
    j = index[i] if r.index.endswith("s") else index[rr]
    assert j.min() >= 0 and j.max() < r.n_dst
    rows = b * r.dst_bstride + j
    assert rows.max() < r.dst_rows
    return rows


def scat_written(r: ScatRow) -> np.ndarray:
    """The block the caller zeroes: every cloud's n_dst rows, C columns."""
    m = np.zeros((r.dst_rows, r.ldd), dtype=bool)
    for b in range(r.B):
        m[b * r.dst_bstride: b * r.dst_bstride + r.n_dst, :r.C] = True
    return m


def scat_initial(r: ScatRow) -> np.ndarray:
    buf = guarded(r.dst_rows * r.ldd, F32)
    buf[GUARD:-GUARD][scat_written(r).reshape(-1)] = 0.0
    return buf


def verify_scat(r: ScatRow, x, index, after, what="") -> float:
    what = what or r.id
    assert silent(after, scat_written(r)), f"{what}: wrote outside the zeroed block"
    rows = scat_dst_rows(r, index)
    v = x[:, r.c0s:r.c0s + r.C].astype(F64)
    ref, S, n = np.zeros((r.dst_rows, r.C)), np.zeros((r.dst_rows, r.C)), np.zeros((r.dst_rows, 1))
    np.add.at(ref, rows, v)
    np.add.at(S, rows, np.abs(v))
    np.add.at(n, rows, 1.0)
    got = after[GUARD:-GUARD].reshape(r.dst_rows, r.ldd)[:, :r.C]
    m = scat_written(r)[:, :r.C]
    return check(got[m], ref[m], (M2 * n * U * S)[m], what)
