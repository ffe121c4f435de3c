"""The gather lattice without a GPU (tests/gather_lattice.py): the tables against the restated host dispatch (every kernel, CAP, TPR,
chunking and instantiation is reached, and the particular numbers the rows were chosen for hold), the restated CSR plan against
rl_csr_workspace_bytes, the host-side refusals of the five entry points (descriptors of aligned dummy pointers: nothing is
launched), and the checkers against the numpy emulations - the faithful ones inside every bound, every mutant rejected.
"""
import ctypes as C

import numpy as np
import pytest

import gather_lattice as G


@pytest.fixture(scope="module")
def HL():
    from randlanet import _hip as H
    return H, H.lib()


@pytest.fixture(scope="module")
def csr_data():
    return [G.make_csr(i) for i in range(len(G.CSR_ROWS))]


# ---- the tables ------------------------------------------------------------------------------------------------------------------
def test_csr_table_reaches_every_kernel_and_border(csr_data):
    reached, by_row = set(), {}
    for i, row in enumerate(G.CSR_ROWS):
        r, t0 = set(), 0
        for chunk in G.csr_chunks(row):
            r |= G.csr_reached(row.B, chunk, csr_data[i][t0:t0 + len(chunk)])
            t0 += len(chunk)
        by_row[row.id] = r
        reached |= r
    want = {"csr2_bucket_kernel<32>", "csr2_bucket_kernel<56>", "csr_sort_kernel<32>", "csr_sort_kernel<64>", "csr_sort_kernel<128>",
            "csr2_sort_long_kernel", "csr2_sort_long_kernel:grid-stride", "csr2_sort_long_kernel:second-chunk", "csr_sort_long_kernel",
            "csr_sort_long_kernel:second-chunk", "csr_sort_kernel:len1", "early-return:tiles", "early-return:buckets", "both-bucket-kernels",
            "dropped", "deal-B2", "deal-B4", "deal-B8"}
    assert want <= reached, want - reached
    assert {"both-bucket-kernels", "early-return:tiles", "early-return:buckets", "deal-B4"} <= by_row["eight-tasks"]
    assert "csr2_sort_long_kernel:grid-stride" in by_row["300-long-segments"]
    assert "csr2_sort_long_kernel:second-chunk" in by_row["one-destination"]
    for B in (1, 2):
        assert {"csr_sort_kernel<32>", "csr_sort_kernel<64>", "csr_sort_kernel<128>", "csr_sort_long_kernel:second-chunk", "dropped",
                "csr_sort_kernel:len1"} <= by_row[f"atomics-B{B}"]
    # the borders the rows were built for
    tasks = {g for row in G.CSR_ROWS for g in row.tasks}
    assert {(g.n_dst, g.per) for g in tasks} >= {(n, e) for n in (1, 255, 256, 257, 513) for e in (1, 4095, 4096, 4097, 8193)}
    assert {row.B for row in G.CSR_ROWS} >= {1, 2, 3, 4, 5, 8}
    assert len(G.CSR_ROWS[[r.id for r in G.CSR_ROWS].index("nine-graphs")].tasks) == 9
    for row in G.CSR_ROWS:
        for chunk in G.csr_chunks(row):
            assert G.csr_plan(row.B, chunk)["two_level"] == (not row.id.startswith("atomics")), row.id
            for g in chunk:
                assert row.B * g.per < 2 ** 31 and row.B * g.n_dst < 2 ** 31


def _lens(data, t):
    return np.diff(data[t][2].astype(np.int64), axis=1)


def test_csr_rows_hold_the_segments_they_name(csr_data):
    ids = [r.id for r in G.CSR_ROWS]
    plan = lambda rid: G.csr_plan(G.CSR_ROWS[ids.index(rid)].B, G.CSR_ROWS[ids.index(rid)].tasks)
    assert plan("mean16-cap32")["tasks"][0]["cap"] == 32 and plan("mean16+-cap56")["tasks"][0]["cap"] == 56
    for rid, cap, a, b in (("len32-33-cap32", 32, 32, 33), ("len56-57-cap56", 56, 56, 57)):
        assert plan(rid)["tasks"][0]["cap"] == cap
        lens = _lens(csr_data[ids.index(rid)], 0)
        assert (lens[:, 0] == a).all() and (lens[:, 1] == b).all() and (lens == 0).any()
    one = csr_data[ids.index("one-destination")]
    assert [int(_lens(one, t).max()) for t in range(3)] == [1024, 1025, 2049] and all((_lens(one, t) > 0).sum() == 2 for t in range(3))
    long = _lens(csr_data[ids.index("300-long-segments")], 0)
    assert (long == 60).all() and long.size == 300 > G.LONG_WGS and plan("300-long-segments")["tasks"][0]["cap"] == 56
    for B in (1, 2):
        p, data = plan(f"atomics-B{B}"), csr_data[ids.index(f"atomics-B{B}")]
        assert not p["two_level"] and p["last_kernel"] == "csr_sort_kernel" and p["need"] == [True, True, True]
        assert [t["cap"] for t in p["tasks"]] == [32, 32, 64, 128]
        for t, cap in ((1, 32), (2, 64), (3, 128)):
            lens = _lens(data, t)
            assert (lens[:, :5] == [0, 1, cap, cap + 1, 1500]).all() and (data[t][4] < data[t][0].per).all()
    eight = plan("eight-tasks")
    assert eight["need"] == [True, True, False] and eight["deal"] and eight["max_tiles"] == 4 and eight["max_buckets"] == 4
    assert min(t["ntiles"] for t in eight["tasks"]) == 1 and min(t["nbuckets"] for t in eight["tasks"]) == 1
    dropped = csr_data[ids.index("dropped")][0]
    flat = dropped[1].reshape(2, -1)
    assert all((flat == v).any() for v in (-1, 1000, G.INT32_MAX, G.INT32_MIN)) and (dropped[4] == 16000 - 1600).all()


def test_segment_sum_table_reaches_every_instantiation():
    d = {r.id: G.seg_dispatch(r) for r in G.SEG_ROWS}
    assert not any(x["refused"] for x in d.values())
    for C, tpr in G.VEC_C:
        assert d[f"vec-C{C}"]["tpr"] == tpr and d[f"vec-C{C}"]["vec"], C
    assert d["vec-C1028"]["column_trips"] == 2 and d["vec-C2048"]["column_trips"] == 2 and d["vec-C1024"]["column_trips"] == 1
    tprs = {(x["tpr"], r.bf16) for r, x in ((r, d[r.id]) for r in G.SEG_ROWS) if x["vec"]}
    assert tprs == {(t, bf) for t in (1, 2, 4, 8, 16, 32, 64, 128, 256) for bf in (False, True)}, sorted(tprs)
    assert any(r.bf16 and d[r.id]["column_trips"] == 2 for r in G.SEG_ROWS)
    for rid in ("scalar-C1", "scalar-C3", "scalar-C10", "scalar-C8-lds10", "scalar-C8-col2", "stride-ldd-scalar"):
        assert d[rid]["kernel"] == "segment_sum_kernel", rid
    assert d["bf16-C16-col4"]["vec"] and d["stride-lds-col"]["vec"] and d["stride-ldd"]["vec"]
    # the chunked rows and their numbers
    for C, B, n_dst, g in G.XCD_ROWS:
        x = d[f"xcd-C{C}-B{B}-n{n_dst}"]
        assert x["g"] == g and x["chunk"] == -(-B * n_dst // 8) and not x["capped"], (C, B, n_dst, x)
    x = d["xcd-C4-B1-n2041"]
    assert x["chunk"] == 256 and 2041 - 7 * 256 == 249
    assert d["xcd-C8-B3-n299"]["chunk"] == 113
    x = d["xcd-C16-B3-n169"]
    assert x["chunk"] == 64 and 507 - 7 * 64 == 59 and 169 % 64 != 0 and x["in_chunk_trips"] == 1
    assert d["xcd-C16-B1-n1021"]["g"] // 8 == 2 and d["xcd-C16-B1-n1021-bf16"]["chunk"] == 128
    x = d["unchunked-C16-total513"]
    assert x["g"] == 9 and x["chunk"] == 0
    x = d["capped-C16-total524289"]
    assert x["capped"] and x["g"] == 8192 and x["chunk"] == 65537 and x["in_chunk_trips"] == 2
    x = d["capped-C512-total16385"]
    assert x["capped"] and x["g"] == 8192 and x["chunk"] == 0 and x["tpr"] == 128
    # the in-degrees, and every cover graph's destinations non-empty
    for i, r in enumerate(G.SEG_ROWS):
        if r.id.startswith("degrees"):
            s = G.make_seg(i)
            assert set(np.diff(s.off[0])) == set(G.DEG_SET) and (np.diff(s.off[0])[:18] == G.DEG_SET).all()
        if r.g.kind == "cover" and not r.big:
            assert (np.diff(G.make_seg(i).off, axis=1) > 0).all(), r.id
    assert {r.C for r in G.SEG_ROWS if r.id.startswith("degrees")} == {4, 16, 64, 1024}
    for name in ("sbs_pad", "dbs_pad", "ldd_pad"):
        assert {r.acc for r in G.SEG_ROWS if getattr(r, name)} == {False, True}, name
    assert {r.acc for r in G.SEG_ROWS if r.col0 and r.lds_pad and not r.bf16} == {False, True}
    perm = G.make_seg([r.id for r in G.SEG_ROWS].index("capped-C512-total16385"))
    lens = np.diff(perm.off[0])
    assert (lens == 0).any() and (lens > 1).any()
    assert all(4 * ((r.dst_rows * r.ldd + r.src_rows * r.lds) + 2 * r.B * r.g.per) < 256 << 20 for r in G.SEG_ROWS)


def test_copy_table_reaches_every_instantiation():
    d = {r.id: G.copy_dispatch(r) for r in G.COPY_ROWS}
    assert len(d) == len(G.COPY_ROWS), "row ids must be unique"
    kernels = {x["kernel"] for x in d.values()}
    assert kernels == {f"copy_rows_kernel<{v}, {t}>" for v in (4, 1) for t in ("uint32_t", "int64_t")}, kernels
    assert d["wide-quad-int64"]["kernel"] == "copy_rows_kernel<4, int64_t>" and d["wide-scalar-int64"]["kernel"] == "copy_rows_kernel<1, int64_t>"
    for rid in ("scalar-C4-col2", "scalar-C8-lds10", "scalar-C8-scale-odd", "scalar-C3-dstcol-ldd"):
        assert d[rid]["vec"] == 1, rid
    assert d["quad-C8-dstcol-ldd"]["vec"] == 4 and d["quad-C8-dstcol-ldd-copy"]["vec"] == 4
    for r in G.COPY_ROWS:
        assert d[r.id]["vec"] == (4 if r.id.startswith(("quad", "capped", "wide-quad")) else 1), r.id
        assert r.src_bstride != r.rows_per_batch
    for v in (4, 1):
        rows = [r for r in G.COPY_ROWS if d[r.id]["vec"] == v]
        assert {r.index for r in rows} == set(G.INDEX_KINDS) and {r.lazy for r in rows} == set(G.LAZY_KINDS), v
        assert {(r.lazy, r.acc) for r in rows} == {(z, a) for z in G.LAZY_KINDS for a in (False, True)}, v
        assert {r.n for r in rows} >= set(G.ROWS_N) and {r.B for r in rows if r.n in G.ROWS_N} == {1, 3}, v
        assert {r.C for r in rows} >= set(G.QUAD_C if v == 4 else G.SCALAR_C), v
    x = d["capped-grid-C64-rows262145"]
    assert x["chunks"] == 4194320 and x["per_trip"] == 4096 * 256 * 4 == 4194304 and x["grid"] == 4096 and x["trips"] == 2
    assert not G.fits32(G.WIDE) and G.fits32(G.WIDE - 1) and G.grid_for(0) == 1 and G.grid_for(4096 * 256 + 1) == 4096
    (a, b, k0), (a1, b1, k1), (a2, b2, k2) = G.PAIR_ROWS
    assert G.pair_eligible(a) and G.pair_eligible(b) and k0 == "copy_rows_pair_kernel" and (a.rows, b.rows) == (2720, 1000) and a.C != b.C
    assert G.pair_eligible(a1) and G.pair_eligible(b1) and not G.pair_eligible(b2) and b2.C == 6 and k2 == "copy_rows_kernel"
    assert {r.index for r in G.SCAT_ROWS} == {"i32", "i64", "i32s", "i64s"} and {r.C for r in G.SCAT_ROWS} == {1, 8}
    assert any(r.wide for r in G.SCAT_ROWS) and any(r.n // r.n_dst >= 800 for r in G.SCAT_ROWS)
    assert all(4 * (r.dst_rows * r.ldd + r.src_rows * r.lds) < 256 << 20 for r in G.COPY_ROWS)


# ---- the restated plan against the library's host side -----------------------------------------------------------------------------------
P = 0x10000000          # a 256-byte-aligned address that is compared and never dereferenced


def _tasks(H, graphs):
    arr = (H.CsrTask * len(graphs))()
    for n, (t, g) in enumerate(zip(arr, graphs)):
        t.idx, t.n_src, t.k, t.n_dst, t.offsets, t.entries = P + n * 0x100000, g.n_src, g.k, g.n_dst, P + 0x8000000 + n * 0x100000, P + 0xC000000 + n * 0x100000
    return arr


def test_restated_plan_gives_the_library_s_workspace_bytes(HL):
    H, L = HL
    for row in G.CSR_ROWS:
        for chunk in G.csr_chunks(row):
            assert L.rl_csr_workspace_bytes(_tasks(H, chunk), len(chunk), row.B) == G.csr_plan(row.B, chunk)["bytes"], row.id
    borders = [G.Graph(8, 1, 262144), G.Graph(8, 1, 262145), G.Graph(2 ** 24 - 1, 1, 1000), G.Graph(2 ** 24, 1, 1000), G.Graph(2 ** 20, 16, 2 ** 20)]
    for n in (600, 1000):
        borders += [G.Graph(n, 16, n), G.Graph(n + 1, 16, n), G.Graph(2 * n, 16, n), G.Graph(2 * n + 1, 16, n), G.Graph(n, 1, 16 * n)]
    assert [G.two_level_ok(g) for g in borders[:4]] == [True, False, True, False]
    for g in borders:
        for B in (1, 3, 8):
            for tasks in ((g,), (g, G.FORCING), (G.Graph(64, 16, 64), g)):
                plan = G.csr_plan(B, tasks)
                assert L.rl_csr_workspace_bytes(_tasks(H, tasks), len(tasks), B) == plan["bytes"], (g, B, len(tasks))
    caps = lambda g, forced: G.csr_plan(1, (g, G.FORCING) if forced else (g,))["tasks"][0]["cap"]
    assert [caps(G.Graph(n, 16, 600), False) for n in (600, 601, 1200, 1201)] == [32, 56, 56, 56]
    assert [caps(G.Graph(n, 16, 600), True) for n in (600, 601, 1200, 1201)] == [32, 64, 64, 128]
    # a cap changes long_cap, and with it the bytes: the equality above would notice a moved border
    assert G.csr_plan(1, (G.Graph(600, 16, 600),))["bytes"] != G.csr_plan(1, (G.Graph(601, 16, 600),))["bytes"] - 64
    assert L.rl_csr_workspace_bytes(_tasks(H, borders[:1]), 0, 1) == 0 and L.rl_csr_workspace_bytes(_tasks(H, borders[:1]), 1, 0) == 0


# ---- refusals: nothing is launched -----------------------------------------------------------------------------------------------------------
def test_host_side_refusals_launch_nothing(HL, monkeypatch):
    H, L = HL
    n0 = L.rl_launch_count()
    ws = P + 0x4000000
    small = (G.Graph(64, 16, 64),)
    need = G.csr_plan(2, small)["bytes"]
    build = lambda graphs, n, B, w=ws, nbytes=1 << 40: L.rl_csr_build(_tasks(H, graphs), n, B, w, nbytes, None)
    assert build(small, 0, 2) == H.ERR_ARGS
    assert build(small * 9, 9, 2) == H.ERR_ARGS
    assert build(small * 8, 8, 8192) == H.ERR_ARGS                            # B * ntasks = 65536
    assert build(small, 1, 2, w=ws + 128) == H.ERR_ARGS and build(small, 1, 2, w=None) == H.ERR_ARGS
    assert build(small, 1, 2, nbytes=need - 1) == H.ERR_ARGS
    assert build((G.Graph(2 ** 20, 16, 2 ** 20),), 1, 128) == H.ERR_ARGS      # B * n_src * k = 2^31
    assert build((G.Graph(64, 16, 0),), 1, 2) == H.ERR_ARGS

    def seg(**kw):
        d = H.SegsumDesc()
        d.src, d.lds, d.src_bstride, d.dst, d.ldd, d.dst_bstride = P, 8, 64, P + 0x100000, 8, 16
        d.offsets, d.entries, d.entries_per_cloud, d.B, d.n_dst, d.C = P + 0x200000, P + 0x300000, 64, 2, 16, 8
        for k, v in kw.items():
            setattr(d, k, v)
        return L.rl_segment_sum_rows(C.byref(d), None)

    assert seg(lds=7) == H.ERR_ARGS and seg(ldd=7) == H.ERR_ARGS
    assert seg(dst_bstride=15) == H.ERR_ARGS
    assert seg(src_bf16=1, C=6) == H.ERR_UNSUPPORTED
    assert seg(src_bf16=1, src=P + 4) == H.ERR_UNSUPPORTED and seg(src_bf16=1, lds=10) == H.ERR_UNSUPPORTED
    assert seg(src=None) == H.ERR_ARGS and seg(C=0) == H.ERR_ARGS and seg(B=1 << 16, n_dst=1 << 15, dst_bstride=1 << 15) == H.ERR_ARGS

    def rows(**kw):
        d = H.RowsDesc()
        d.src, d.lds, d.src_bstride, d.dst, d.ldd, d.rows, d.rows_per_batch, d.C = P, 8, 64, P + 0x100000, 8, 128, 64, 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    i32, i64 = P + 0x200000, P + 0x300000
    for fn in (L.rl_copy_rows, L.rl_scatter_add_rows):
        assert fn(C.byref(rows(index32=i32, index64=i64)), None) == H.ERR_ARGS
        assert fn(C.byref(rows(index32=i32, scale=P + 0x400000)), None) == H.ERR_ARGS
        assert fn(C.byref(rows(index32=i32, shift=P + 0x400000)), None) == H.ERR_ARGS
        assert fn(C.byref(rows(index32=i32, C=0)), None) == H.ERR_ARGS and fn(C.byref(rows(index32=i32, rows_per_batch=0)), None) == H.ERR_ARGS
    assert L.rl_copy_rows_pair(C.byref(rows()), C.byref(rows(index32=i32, index64=i64)), None) == H.ERR_ARGS
    assert L.rl_copy_rows(C.byref(rows(rows=0)), None) == 0                  # nothing to move: accepted, nothing launched
    monkeypatch.delenv("RL_ALLOW_FLOAT_ATOMICS", raising=False)
    assert L.rl_scatter_add_rows(C.byref(rows()), None) == H.ERR_ARGS         # no index
    assert L.rl_scatter_add_rows(C.byref(rows(index32=i32)), None) == H.ERR_UNSUPPORTED
    monkeypatch.setenv("RL_ALLOW_FLOAT_ATOMICS", "1")
    assert L.rl_scatter_add_rows(C.byref(rows()), None) == H.ERR_ARGS
    assert L.rl_scatter_add_rows(C.byref(rows(index32=i32, scale=P + 0x400000, shift=P + 0x500000)), None) == H.ERR_ARGS
    assert L.rl_scatter_add_rows(C.byref(rows(index32=i32, rows=0)), None) == 0
    assert L.rl_launch_count() == n0


# ---- the checkers against the emulations ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for fam, (ratio, where) in sorted(w.items()):
        print(f"[gather lattice emulation] {fam:<14} max error / bound {ratio:.3f}  ({where})")


def _note(w, fam, ratio, where):
    if ratio >= w.get(fam, (-1.0, ""))[0]:
        w[fam] = (ratio, where)


SEG_CPU = [i for i, r in enumerate(G.SEG_ROWS) if not r.big]
COPY_CPU = [i for i, r in enumerate(G.COPY_ROWS) if not r.big]


def test_bf16_rounding_is_torch_s():
    import torch
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * np.float32(37.0)
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]                                   # ties: to even
    t = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(G.bf16_round(x), t.float().numpy())
    assert np.array_equal(G.bf16_bits(G.bf16_round(x)), t.view(torch.int16).numpy())


def test_csr_emulation_matches_the_reference_and_mutants_are_rejected(csr_data):
    rejected = {m: 0 for m in G.CSR_MUTANTS}
    for i, row in enumerate(G.CSR_ROWS):
        for t, (g, idx, off, ent, kept) in enumerate(csr_data[i]):
            if g.n_dst > 100000:
                continue
            G.verify_csr(g, off, ent, kept, *G.emulate_csr(g, idx), what=f"{row.id} task {t}")
            for m in G.CSR_MUTANTS:
                try:
                    G.verify_csr(g, off, ent, kept, *G.emulate_csr(g, idx, m))
                except AssertionError:
                    rejected[m] += 1
    assert all(n > 0 for n in rejected.values()), rejected
    # a write into a guard band is noticed
    g, idx, off, ent, kept = csr_data[0][0]
    ob, eb = G.emulate_csr(g, idx)
    eb[-1] = 0
    with pytest.raises(AssertionError, match="outside"):
        G.verify_csr(g, off, ent, kept, ob, eb)


@pytest.mark.parametrize("i", SEG_CPU, ids=[G.SEG_ROWS[i].id for i in SEG_CPU])
def test_segment_sum_emulation_is_inside_its_bound(worst, i):
    s = G.make_seg(i)
    G.seg_indices_in_range(s)
    _note(worst, "segment_sum" + (" bf16" if s.row.bf16 else ""), G.verify_seg(s, G.emulate_seg(s)), s.row.id)


@pytest.mark.parametrize("mutant", G.SEG_MUTANTS)
def test_segment_sum_checker_rejects_the_mutant(mutant):
    rejected, by_order_only = [], []
    for i in SEG_CPU:
        s = G.make_seg(i)
        bad = G.emulate_seg(s, mutant)
        try:
            G.verify_seg(s, bad)
        except AssertionError as e:
            rejected.append(s.row.id)
            if "segment order" in str(e):
                by_order_only.append(s.row.id)
    assert rejected, mutant
    if mutant == "descending":      # inside the fp64 bound (any order is), caught by the order contract alone
        assert by_order_only and by_order_only == rejected, (rejected, by_order_only)
    if mutant == "first_row_of_chunk_skipped":
        assert all(G.seg_dispatch(G.SEG_ROWS[[r.id for r in G.SEG_ROWS].index(rid)])["chunk"] for rid in rejected)
        assert len(rejected) == sum(1 for i in SEG_CPU if G.seg_dispatch(G.SEG_ROWS[i])["chunk"])
    if mutant == "src_bstride_off_by_one":
        assert len(rejected) == sum(1 for i in SEG_CPU if G.SEG_ROWS[i].B > 1)
    if mutant == "accumulate_dropped":
        assert len(rejected) == sum(1 for i in SEG_CPU if G.SEG_ROWS[i].acc)


def test_segment_sum_checker_notices_a_csr_defect_and_a_stray_write():
    i = [r.id for r in G.SEG_ROWS].index("degrees-C16-fp32")
    s = G.make_seg(i)
    for m in G.CSR_MUTANTS[1:]:
        ob, eb = G.emulate_csr(s.row.g, s.idx, m)
        off = np.minimum(ob[G.GUARD:-G.GUARD].reshape(s.off.shape), s.row.g.per)
        with pytest.raises(AssertionError):
            G.verify_seg(s, G.emulate_seg(s, off=off, ent=eb[G.GUARD:-G.GUARD].reshape(s.ent.shape)))
    for where in (0, G.GUARD + s.row.total * s.row.ldd, -1):      # front guard, the row after the last one, back guard
        buf = G.emulate_seg(s)
        buf[where] = 0.0
        with pytest.raises(AssertionError, match="outside"):
            G.verify_seg(s, buf)


@pytest.mark.parametrize("i", COPY_CPU, ids=[G.COPY_ROWS[i].id for i in COPY_CPU])
def test_copy_emulation_is_inside_its_bound(worst, i):
    c = G.make_copy(G.COPY_ROWS[i], G.seed(3, i))
    _note(worst, "copy_rows" + ("" if c.row.lazy == "none" else " lazy"), G.verify_copy(c, G.emulate_copy(c)), c.row.id)


@pytest.mark.parametrize("mutant", G.COPY_MUTANTS)
def test_copy_checker_rejects_the_mutant(mutant):
    rejected = 0
    for i in COPY_CPU:
        c = G.make_copy(G.COPY_ROWS[i], G.seed(3, i))
        try:
            G.verify_copy(c, G.emulate_copy(c, mutant))
        except AssertionError:
            rejected += 1
    want = sum(1 for i in COPY_CPU if (G.COPY_ROWS[i].acc if mutant == "accumulate_dropped" else G.COPY_ROWS[i].B > 1))
    assert rejected == want > 0, (mutant, rejected, want)


def test_copy_checker_tells_the_activations_apart():
    """A ReLU row computed as LeakyReLU (and the reverse) is outside the bound; -0 for +0 is accepted (by value)."""
    ids = [r.id for r in G.COPY_ROWS]
    for rid, other in (("quad-C8-i32-relu-acc", "lrelu"), ("scalar-C6-i32-lrelu", "relu")):
        i = ids.index(rid)
        c = G.make_copy(G.COPY_ROWS[i], G.seed(3, i))
        swapped = G.Copy(G.CopyRow(**{**c.row.__dict__, "lazy": other}), c.x, c.index, c.scale, c.shift, c.old)
        with pytest.raises(AssertionError):
            G.verify_copy(c, G.emulate_copy(swapped))
    i = ids.index("quad-C8-none-relu")
    c = G.make_copy(G.COPY_ROWS[i], G.seed(3, i))
    buf = G.emulate_copy(c)
    body = buf[G.GUARD:-G.GUARD]
    zeros = (body == 0.0) & (body.view(np.int32) != G.SENT)
    assert zeros.any()
    body[zeros] = np.float32(0.0) * np.float32(-1.0) * body[zeros]      # flip the zeros' signs
    G.verify_copy(c, buf)


def test_scatter_checker():
    for i in range(len(G.SCAT_ROWS)):
        r, x, index = G.make_scat(i)
        buf = G.scat_initial(r)
        body = buf[G.GUARD:-G.GUARD].reshape(r.dst_rows, r.ldd)
        rows = G.scat_dst_rows(r, index)
        order = np.random.default_rng(i).permutation(r.rows)                 # any order
        for c in range(r.C):
            col = np.zeros(r.dst_rows, dtype=np.float32)
            for e in order:
                col[rows[e]] += x[e, r.c0s + c]
            body[:, c] = np.where(G.scat_written(r)[:, c], col, body[:, c])
        assert G.verify_scat(r, x, index, buf) <= 1.0
        lost = buf.copy()
        lost[G.GUARD:-G.GUARD].reshape(r.dst_rows, r.ldd)[rows[order[-1]], 0] -= x[order[-1], r.c0s]     # one contribution lost
        with pytest.raises(AssertionError):
            G.verify_scat(r, x, index, lost)
