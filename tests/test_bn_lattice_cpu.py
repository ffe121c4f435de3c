"""The BatchNorm lattice without a GPU (tests/bn_lattice.py): the table's self-checks, the activation-sign condition of every
row, the host-only entry points of csrc/bn.hip at their borders (descriptors of 16-byte-aligned dummy pointers: every call here
is refused or answered on the host, nothing is launched), and the checker against the emulation - the faithful one inside every
bound of every row, each of the twelve mutants rejected on at least one row.
"""
import ctypes as C

import numpy as np
import pytest

import bn_lattice as B


@pytest.fixture(scope="module")
def HL():
    from randlanet import _hip as H
    return H, H.lib()


ROWS = [(i, j) for i, c in enumerate(B.CASES) for j in range(len(c.edges))]


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_kernel_and_every_option_meets_every_family():
    reached = set()
    seen = {}
    for i, c in enumerate(B.CASES):
        for j, e in enumerate(c.edges):
            r = B.sm_r(e.M) if c.family in ("small", "resid_small") else 0
            reached |= {(k, r) for k in c.kernels}
            seen.setdefault(c.family, []).append(B.options(i, j))
            # the row's kernel is the one the dispatch of bn.hip picks for it
            if c.family == "vec":
                assert B.vec_eligible(c.C) and c.lda % 4 == 0 and c.misalign is None, c.id
            if c.family == "scalar":
                assert not (B.vec_eligible(c.C) and c.lda % 4 == 0 and c.misalign is None), c.id
            if c.family in ("small", "resid_small"):
                assert e.M <= B.SM_ROWS and c.C % 4 == 0 and c.lda % 4 == 0, c.id
            if c.family.startswith("resid"):
                assert B.vec_eligible(c.C) and e.bstride == e.n and c.lda == c.C, c.id
            assert e.bstride >= e.n and c.lda >= c.C
    print("[bn lattice] kernels reached:", sorted(reached))
    assert reached == B.REACHED
    for fam, opts in seen.items():
        if not fam.startswith("resid"):
            assert {o.act for o in opts} == {0, 1, 2}, fam
            assert {o.affine for o in opts} == {False, True}, fam
            assert {(o.act, o.affine) for o in opts} == {(a, f) for a in (0, 1, 2) for f in (False, True)}, fam
        else:
            assert {o.resid_slope for o in opts} == {0.01, 0.0}, fam
        if fam in ("vec", "scalar"):
            assert {o.items for o in opts} == {1, 2, 8}, fam
        if fam == "small":
            assert {o.count3 for o in opts} == {False, True}, fam
    # the sets of the specification
    C_of = lambda fam: {c.C for c in B.CASES if c.family == fam}
    assert C_of("vec") >= {4, 8, 128, 256, 512, 1024} and C_of("scalar") >= {1, 3, 6, 10, 12, 100, 255, 257, 300, 1023}
    assert C_of("small") >= {4, 8, 12, 24, 36, 64, 1024} and C_of("resid_sweep") == C_of("resid_small") == {4, 32, 256, 1024}
    assert {B.lanes("vec", C_)[0] for C_ in (4, 8, 128, 256, 512, 1024)} == {1, 2, 32, 64, 128, 256}
    for c in B.CASES:
        if c.id.startswith(("vec_c", "scalar_c", "resid_sweep_c")):
            rpar = B.lanes("scalar" if c.family == "scalar" else "vec", c.C)[1]
            want = {M for M in (1, rpar - 1, rpar, rpar + 1, 2 * rpar + 1, 15, 16, 17) if M >= 1}
            assert want <= {e.M for e in c.edges}, c.id
        if c.id.startswith(("small_c", "resid_small_c")):
            assert {e.M for e in c.edges} == set(B.SMALL_ROWS), c.id
    for fam in ("vec", "scalar", "small"):
        mine = [c for c in B.CASES if c.family == fam]
        assert any(c.ld > c.C for c in mine) and any(e.bstride > e.n for c in mine for e in c.edges), fam
        assert any(B.STRIDED in c.edges for c in mine), fam
    assert {c.misalign for c in B.CASES} == {None, "base", "vectors"}
    by_id = {c.id: c for c in B.CASES}
    for cid, M in (("vec_grid_16385x4", 16385), ("scalar_grid_16385x3", 16385), ("vec_grid_65537x8", 65537), ("vec_grid_524289x4", 524289),
                   ("resid_grid_16385x4", 16385)):
        assert by_id[cid].edges[0].M == M and B.slots(M) == B.MAX_SLOTS
    assert (B.bn_tile(16385), B.bn_tile(65537), B.bn_tile(524289)) == (16, 32, 256)
    # C = 36: nine quads on sixteen workgroups, two per XCD and a short last one; every quad owned exactly once
    for C_ in (4, 8, 12, 24, 36, 64, 1024):
        q = [x for x in B.small_quads(C_) if x >= 0]
        assert sorted(q) == list(range(C_ // 4)), C_
    assert B.small_quads(36).count(-1) == 7
    # the fold table
    assert {f.nslots for f in B.FOLDS} >= {1, 255, 256, 257, 1024} and {f.C for f in B.FOLDS} >= {1, 5, 64, 1024}
    for want in (dict(bias=True), dict(pivot="running"), dict(pivot="vector"), dict(training=False), dict(training=False, bias=True),
                 dict(count=1), dict(clamp=True), dict(affine=False), dict(running=False)):
        assert any(all(getattr(f, k) == v for k, v in want.items()) for f in B.FOLDS), want
    items = B.batch_items(49)
    assert {it.C for it in items} >= {1, 1024} and {it.training for it in items} == {False, True}


def test_sum_depth_is_the_layouts():
    assert B.sum_depth("vec", 4, 17) == 1 + 6           # one row per lane per tile, one tile per workgroup, six butterfly steps
    assert B.sum_depth("vec", 1024, 17) == 16           # rpar = 1: sixteen rows per lane
    assert B.sum_depth("vec", 128, 17) == 2 + 1         # rpar = 8, one butterfly step
    assert B.sum_depth("vec", 4, 16385) == 2 + 6        # 1025 tiles on 1024 workgroups
    assert B.sum_depth("vec", 4, 524289) == 3 + 6       # 2049 tiles of 256 rows
    assert B.sum_depth("scalar", 3, 16385) == 2
    assert B.sum_depth("scalar", 300, 17) == 16
    assert B.sum_depth("small", 8, 1024) == 7 and B.sum_depth("resid_small", 8, 1025) == 8


@pytest.mark.parametrize("i", range(len(B.CASES)), ids=[c.id for c in B.CASES])
def test_activation_signs_are_unambiguous(i):
    case = B.CASES[i]
    for j in range(len(case.edges)):
        if case.edges[j].M * case.C > 1 << 19:
            continue                                    # (the large rows are made - and asserted - once, in the emulation test)
        inp = B.make_bwd(case, i, j)                   # asserts on the way out
        B.assert_signs(inp)
        if not inp.resid and "scale" in inp.a:
            assert int(B.sign_margin(inp.logical("Y"), inp.a["scale"], inp.a["shift"]).sum()) == 0
        for name in ("G", "Y", "O", "Y1", "Y2"):
            if name in inp.a:
                s = inp.a[name]
                assert np.isfinite(inp.logical(name)).all() and int(np.isnan(s).sum()) == s.size - inp.M * case.C


# ---- the host-only entry points ----------------------------------------------------------------------------------------------------------------
def test_slots_and_support_queries_at_their_borders(HL):
    H, L = HL
    want = {1: 1, 16: 1, 17: 2, 16384: 1024, 16385: 1024, 65536: 1024, 65537: 1024, 524288: 1024, 524289: 1024}
    for rows, n in want.items():
        assert L.rl_bn_bwd_slots(rows) == n == B.slots(rows), rows
    for rows in (15, 31, 33, 4096, 16383, 70000, 131073, 300000, 1 << 22):
        assert L.rl_bn_bwd_slots(rows) == B.slots(rows), rows
    fused = L.rl_bn_bwd_fused_supported
    assert [fused(r, 8, 8) for r in (0, 1, 2048, 2049)] == [0, 1, 1, 0]
    assert [fused(64, c, c) for c in (0, 4, 6, 12, 36, 1024)] == [0, 1, 0, 1, 1, 1]
    assert [fused(64, 8, ld) for ld in (8, 9, 10, 12, 24)] == [1, 0, 0, 1, 1]
    resid, rfused = L.rl_resid_bn_bwd_supported, L.rl_resid_bn_bwd_fused_supported
    assert [resid(100, c) for c in (0, 2, 4, 8, 12, 32, 36, 256, 1024, 1028, 2048)] == [0, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0]
    assert [resid(r, 32) for r in (0, 1, (1 << 31) - 1, 1 << 31)] == [0, 1, 1, 0]
    assert [rfused(r, 32) for r in (0, 1, 2048, 2049)] == [0, 1, 1, 0] and rfused(64, 12) == 0


P = 0x10000000          # a 16-byte-aligned address that is compared and never dereferenced


def _desc(H, **kw):
    d = H.BnBwdDesc()
    d.G, d.Y, d.ld, d.bstride, d.B, d.n, d.C, d.act = P, P + 0x100000, 8, 64, 1, 64, 8, 0
    d.scale, d.shift, d.mean, d.invstd, d.stats, d.coef = (P + 0x200000 + 0x1000 * k for k in range(6))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_descriptor_refusals_launch_nothing(HL):
    H, L = HL
    n0 = L.rl_launch_count()
    out = [P + 0x300000 + 0x1000 * k for k in range(4)]

    def fused(**kw):
        d = _desc(H, **kw)
        return L.rl_bn_bwd_fused(C.byref(d), d.B * d.n, out[0], out[1], out[2], None)

    assert fused(n=2049, bstride=2049) == H.ERR_UNSUPPORTED
    assert fused(C=6) == H.ERR_UNSUPPORTED
    assert fused(ld=10) == H.ERR_UNSUPPORTED
    assert fused(C=1028, ld=1028) == H.ERR_ARGS
    for name in ("scale", "shift", "mean", "invstd"):
        assert fused(**{name: P + 0x200004}) == H.ERR_ARGS, name
    assert fused(G=P + 4) == H.ERR_UNSUPPORTED and fused(mean=None) == H.ERR_ARGS
    for fn in (L.rl_bn_bwd_reduce, L.rl_bn_bwd_apply):
        for kw in (dict(C=0), dict(C=1025, ld=1025), dict(ld=7), dict(bstride=63), dict(G=None), dict(B=1 << 16, n=1 << 15, bstride=1 << 15)):
            assert fn(C.byref(_desc(H, **kw)), None) == H.ERR_ARGS, kw
    assert L.rl_bn_bwd_reduce(C.byref(_desc(H, stats=None)), None) == H.ERR_ARGS
    assert L.rl_bn_bwd_apply(C.byref(_desc(H, mean=None)), None) == H.ERR_ARGS
    # the junction
    r = H.ResidBnBwdDesc()
    r.G, r.G2, r.O, r.rows, r.C, r.Y1, r.Y2 = P, P + 0x100000, P + 0x200000, 64, 12, P + 0x300000, P + 0x400000
    r.scale1, r.mean1, r.invstd1, r.scale2, r.mean2, r.invstd2, r.stats1, r.stats2, r.coef1, r.coef2 = (P + 0x500000 + 0x1000 * k for k in range(10))
    for fn in (L.rl_resid_bn_bwd_reduce, L.rl_resid_bn_bwd_apply):
        assert fn(C.byref(r), None) == H.ERR_UNSUPPORTED
    assert L.rl_resid_bn_bwd_fused(C.byref(r), *out, None) == H.ERR_UNSUPPORTED
    r.C, r.rows = 32, 2049
    assert L.rl_resid_bn_bwd_fused(C.byref(r), *out, None) == H.ERR_UNSUPPORTED
    r.rows, r.mean2 = 64, P + 0x500004
    assert L.rl_resid_bn_bwd_fused(C.byref(r), *out, None) == H.ERR_ARGS
    # finalizers: nine items, no items, an item without coef
    items = (H.BnBwdFinalizeItem * 9)()
    for it in items:
        it.stats, it.count, it.coef, it.nslots, it.C = P, 64, P + 0x1000, 1, 8
    assert L.rl_bn_bwd_finalize_batch(items, 9, None) == H.ERR_ARGS and L.rl_bn_bwd_finalize_batch(items, 0, None) == H.ERR_ARGS
    items[1].coef = None
    assert L.rl_bn_bwd_finalize_batch(items, 2, None) == H.ERR_ARGS
    assert L.rl_bn_bwd_finalize(P, 0, 64, 8, None, None, P, None) == H.ERR_ARGS
    assert L.rl_bn_bwd_finalize_pair(P, None, 1, 64, 8, None, None, P, None, None, P, None) == H.ERR_ARGS
    assert L.rl_bn_reduce_slots(P, 0, 8, P, None) == H.ERR_ARGS
    # the forward fold: eval without running buffers, pivoted statistics in eval, training without partials
    fin = lambda **kw: L.rl_bn_finalize(*[kw.get(k, v) for k, v in (
        ("stats", P), ("nslots", 1), ("count", 64), ("C", 8), ("gamma", None), ("beta", None), ("rmean", P), ("rvar", P), ("nbt", None),
        ("momentum", 0.99), ("eps", 1e-6), ("training", 1), ("scale", P), ("shift", P), ("save_mean", None), ("save_invstd", None),
        ("bias", None), ("pivoted", 0), ("pivot", None), ("stream", None))])
    assert fin(training=0, rmean=None) == H.ERR_ARGS and fin(training=0, pivoted=1) == H.ERR_ARGS
    assert fin(pivoted=1, rmean=None, rvar=None) == H.ERR_ARGS and fin(stats=None) == H.ERR_ARGS and fin(count=0) == H.ERR_ARGS
    assert fin(scale=None) == H.ERR_ARGS
    fit = (H.BnFinalizeItem * 2)()
    assert L.rl_bn_finalize_batch(fit, 2, None) == H.ERR_ARGS and L.rl_bn_finalize_batch(None, 1, None) == H.ERR_ARGS
    assert L.rl_launch_count() == n0


# ---- the checker against the emulation -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for fam, (ratio, where) in sorted(w.items()):
        print(f"[bn lattice emulation] {fam:<12} max error / bound {ratio:.3f}  ({where})")


@pytest.mark.parametrize("i", range(len(B.CASES)), ids=[c.id for c in B.CASES])
def test_faithful_emulation_is_inside_every_bound(worst, i):
    case = B.CASES[i]
    for j in range(len(case.edges)):
        inp = B.make_bwd(case, i, j)
        ratios = B.verify_bwd(inp, B.emulate_bwd(inp))
        top = max(ratios, key=ratios.get)
        if ratios[top] >= worst.get(case.family, (-1, ""))[0]:
            worst[case.family] = (ratios[top], f"{case.id} {case.edges[j]} {top}")


def _row(cid):
    return next(i for i, c in enumerate(B.CASES) if c.id == cid)


def _edges_where(cid, pred):
    i = _row(cid)
    return [(i, j) for j in range(len(B.CASES[i].edges)) if pred(B.CASES[i].edges[j], B.options(i, j))]


# where each mutant must show: rows of the table chosen from the mutant's meaning, never from a kernel's result
MUTANT_ROWS = {
    "tail_dropped": lambda: _edges_where("vec_c1024", lambda e, o: e.M in (15, 17)) + _edges_where("vec_c8", lambda e, o: e.M == 257),
    "no_grid_stride": lambda: [(_row("vec_grid_16385x4"), 0), (_row("scalar_grid_16385x3"), 0), (_row("resid_grid_16385x4"), 0)],
    "bstride_ignored": lambda: [(_row(c), 0) for c in ("vec_strided", "scalar_strided", "small_strided")],
    # (a single row may be positive in every channel: the ReLU edges of fifteen rows and more)
    "relu_as_lrelu": lambda: [(i, j) for i, j in ROWS if B.CASES[i].id in ("vec_c8", "scalar_c10", "small_c12") and B.options(i, j).act == 1
                              and B.CASES[i].edges[j].M >= 15],
    "coef_swapped": lambda: _edges_where("vec_c128", lambda e, o: e.M >= 15) + _edges_where("scalar_c100", lambda e, o: e.M >= 15),
    "xhat_without_invstd": lambda: _edges_where("vec_c256", lambda e, o: e.M >= 15) + _edges_where("scalar_c12", lambda e, o: e.M >= 15),
    "local_rows_for_count": lambda: [(i, j) for i, j in ROWS if B.CASES[i].id == "small_c24" and B.options(i, j).count3],
    "last_quad_unowned": lambda: [(_row("small_c36"), j) for j in range(len(B.SMALL_ROWS))],
    "second_channel_pass_skipped": lambda: [(_row(c), 0) for c in ("scalar_c257", "scalar_c300", "scalar_c1023")],
}


@pytest.mark.parametrize("mutant", B.MUTANTS_BWD)
def test_checker_rejects_the_backward_mutant(mutant):
    where = MUTANT_ROWS[mutant]()
    assert where, mutant
    rejected = 0
    for i, j in where:
        inp = B.make_bwd(B.CASES[i], i, j)
        B.verify_bwd(inp, B.emulate_bwd(inp))                  # the faithful emulation passes the very row ...
        try:
            B.verify_bwd(inp, B.emulate_bwd(inp, mutant))      # ... on which the mutant is rejected
        except AssertionError as e:
            assert "x its bound" in str(e) or "non-finite" in str(e) or "outside the addressed block" in str(e), e
            rejected += 1
    print(f"[bn lattice] {mutant}: rejected on {rejected} of {len(where)} rows")
    assert rejected == len(where), f"{mutant}: passed on {len(where) - rejected} of the rows chosen to show it"


@pytest.mark.parametrize("k", range(len(B.FOLDS)), ids=[f.id for f in B.FOLDS])
def test_faithful_fold_emulation_is_inside_every_bound(worst, k):
    f = B.FOLDS[k]
    a = B.make_fold(f, k)
    ratios = B.verify_fold(f, a, B.emulate_fold(f, a))
    top = max(ratios, key=ratios.get)
    if ratios[top] >= worst.get("fold", (-1, ""))[0]:
        worst["fold"] = (ratios[top], f"{f.id} {top}")


FOLD_MUTANT_ROWS = {
    "unbiased_factor_missing": ("plain_s1_c5", "plain_s1_c1"),          # n = 4: the factor is 4 / 3
    "pivot_not_added": ("pivot_running_s256_c5", "pivot_vector_s1024_c64", "pivot_vector_bias_s257_c1024"),
    "bias_missing_from_running_mean": ("bias_s257_c64", "pivot_running_bias_s255_c64", "count1_bias_s1_c64"),
}


@pytest.mark.parametrize("mutant", B.MUTANTS_FOLD)
def test_checker_rejects_the_fold_mutant(mutant):
    for fid in FOLD_MUTANT_ROWS[mutant]:
        k = next(k for k, f in enumerate(B.FOLDS) if f.id == fid)
        f = B.FOLDS[k]
        a = B.make_fold(f, k)
        B.verify_fold(f, a, B.emulate_fold(f, a))
        with pytest.raises(AssertionError, match="x its bound"):
            B.verify_fold(f, a, B.emulate_fold(f, a, mutant))


def test_batch_items_and_slot_sums_emulation():
    for count in B.FOLD_BATCHES:
        for k, f in enumerate(B.batch_items(count)):
            a = B.make_fold(f, 100 * count + k)
            B.verify_fold(f, a, B.emulate_fold(f, a))
    for k, (ns, C_) in enumerate(B.SLOT_CASES):
        x = np.random.default_rng(k).standard_normal((ns, 2, C_)) * 100.0
        ref, bound = B.reference_slots(x)
        got = np.stack([B.slot_sums_wave(x[:, 0]), B.slot_sums_wave(x[:, 1])])
        B.check(got, ref, bound, f"slots {ns} x {C_}")
        with pytest.raises(AssertionError):                     # a slot left out is far outside nslots . 2^-53
            B.check(got - x[ns - 1], ref, bound, "last slot dropped")
