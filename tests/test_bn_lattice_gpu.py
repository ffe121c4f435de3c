"""Every kernel of csrc/bn.hip on the MI355X against fp64, per channel and per element.

One case per row of tests/bn_lattice.py.  At each edge of a row the launch sequence goes through the C ABI's descriptors (reduce ->
the three finalizers -> apply with and without coefficients; or the one-launch form; or the junction's), with the kernel
rl_last_kernel names and rl_launch_count asserted after every call, every output held to the bounds of the module's docstring,
everything outside the addressed block (NaN before the launch) bit for bit what it was, and a second run bit-equal to the
first - through ops.bn_backward / ops.resid_bn_backward wherever their dispatch expresses the row, else through the descriptor
again.  The three-launch path and the one-launch path are each held to fp64, never to each other.  The forward fold, its batch
form and rl_bn_reduce_slots are fed double partials the test writes.  No element is excluded from any comparison.

The largest error / bound per kernel family, and the file's wall time, are printed when the module is done.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import bn_lattice as B

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from randlanet import _ops
    return _ops


@pytest.fixture(scope="module")
def H():
    from randlanet import _hip
    return _hip


@pytest.fixture(scope="module")
def report():
    worst, t0 = {}, time.perf_counter()
    yield worst
    for fam, (ratio, where) in sorted(worst.items()):
        print(f"[bn lattice] {fam:<16} max error / bound {ratio:.3f}  ({where})")
    print(f"[bn lattice] wall time {time.perf_counter() - t0:.1f} s")


def _note(report, fam, ratios, where):
    """The worst ratio per family: the per-channel sums (dbeta, dgamma, coef), the apply without coefficients, and the rest (dY)."""
    for name, ratio in ratios.items():
        key = f"{fam} sums" if fam in B.KERNELS and name.startswith(("dbeta", "dgamma", "coef")) else fam
        key = f"{fam} act only" if name == "dY_act" else key
        if ratio >= report.get(key, (-1.0, ""))[0]:
            report[key] = (ratio, f"{where} {name}")


def place(x, off=0):
    """A numpy array on the device, `off` floats past a 16-byte boundary (a view into a larger buffer)."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def filled(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


class Calls:
    """The library with the launch count and the kernel name asserted after every call."""

    def __init__(self, H, where):
        self.H, self.L, self.where = H, H.lib(), where

    def __call__(self, name, *args, kernel=None, launches=1):
        fn = getattr(self.L, name)
        n0 = self.L.rl_launch_count()
        rc = fn(*args, self.H.stream_ptr())
        assert rc == 0, (self.where, name, rc, self.L.rl_last_error())
        assert self.L.rl_launch_count() == n0 + launches, (self.where, name)
        if kernel is not None:
            assert self.L.rl_last_kernel().decode() == kernel, (self.where, name, self.L.rl_last_kernel())


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)


def _finalizers(call, H, stats_list, ns, count, Cc, items):
    """rl_bn_bwd_finalize, _pair and _batch on the same partials: bit-equal to one another; returns [(dgamma, dbeta, coef)] per stats."""
    def outs():
        return [(filled((Cc,), 7.0), filled((Cc,), 7.0), filled((2 * Cc,), 7.0)) for _ in stats_list]

    single = outs()
    for st, (dg, db, co) in zip(stats_list, single):
        call("rl_bn_bwd_finalize", st.data_ptr(), ns, count, Cc, dg.data_ptr(), db.data_ptr(), co.data_ptr())
    s0, s1 = (stats_list * 2)[:2]                                # (one BatchNorm: the pair finalizes the same partials twice)
    pair = [(filled((Cc,), 7.0), filled((Cc,), 7.0), filled((2 * Cc,), 7.0)) for _ in range(2)]
    call("rl_bn_bwd_finalize_pair", s0.data_ptr(), s1.data_ptr(), ns, count, Cc, pair[0][0].data_ptr(), pair[0][1].data_ptr(),
         pair[0][2].data_ptr(), pair[1][0].data_ptr(), pair[1][1].data_ptr(), pair[1][2].data_ptr())
    batch = [(filled((Cc,), 7.0), filled((Cc,), 7.0), filled((2 * Cc,), 7.0)) for _ in range(items)]
    arr = (H.BnBwdFinalizeItem * items)()
    for k, (it, (dg, db, co)) in enumerate(zip(arr, batch)):
        it.stats, it.count, it.dgamma, it.dbeta, it.coef = stats_list[k % len(stats_list)].data_ptr(), count, dg.data_ptr(), db.data_ptr(), co.data_ptr()
        it.nslots, it.C = ns, Cc
    call("rl_bn_bwd_finalize_batch", arr, items)
    for k, trio in enumerate(pair):
        for x, y in zip(trio, single[k % len(single)]):
            assert torch.equal(x, y), (call.where, "finalize_pair differs from finalize")
    for k, trio in enumerate(batch):
        for x, y in zip(trio, single[k % len(single)]):
            assert torch.equal(x, y), (call.where, "finalize_batch differs from finalize")
    return single


def _bwd_desc(H, inp, G, Y, v):
    c, e, o = inp.case, inp.edge, inp.opts
    d = H.BnBwdDesc()
    d.G, d.Y, d.ld, d.bstride, d.B, d.n, d.C = G.data_ptr(), Y.data_ptr(), c.lda, e.bstride, e.B, e.n, c.C
    d.act, d.slope = o.act, B.SLOPE if o.act == B.ACT_LRELU else 0.0
    d.scale, d.shift, d.mean, d.invstd = H.ptr(v.get("scale")), H.ptr(v.get("shift")), v["mean"].data_ptr(), v["invstd"].data_ptr()
    return d


def _plain_edge(ops, H, report, case, i, j):
    inp = B.make_bwd(case, i, j)
    ref = B.reference_bwd(inp)
    L = H.lib()
    e, o, Cc, M = inp.edge, inp.opts, case.C, inp.M
    where = f"{case.id} {e}"
    call = Calls(H, where)
    base = 1 if case.misalign == "base" else 0
    voff = 1 if case.misalign == "vectors" else 0
    Y = place(inp.a["Y"], base)
    v = {k: place(inp.a[k], voff if k in ("scale", "mean") else 0) for k in ("scale", "shift", "mean", "invstd") if k in inp.a}
    small = case.family == "small"
    fused_ok = bool(L.rl_bn_bwd_fused_supported(M, Cc, case.lda))
    assert fused_ok or not small

    def by_descriptor():
        G = place(inp.a["G"], base)
        d = _bwd_desc(H, inp, G, Y, v)
        got = {}
        if small:
            dg, db = filled((Cc,), 7.0), filled((Cc,), 7.0)
            co = filled((2 * Cc,), 7.0) if o.count3 else None
            call("rl_bn_bwd_fused", C.byref(d), inp.count, dg.data_ptr(), db.data_ptr(), H.ptr(co), kernel=case.kernels[0])
            if co is not None:
                got["coef"] = co.cpu().numpy()
        else:
            ns = B.slots(M)
            assert L.rl_bn_bwd_slots(M) == ns, where
            stats = filled((ns + 1, 2, Cc), float("nan"), torch.float64)
            d.stats = stats.data_ptr()
            call("rl_bn_bwd_reduce", C.byref(d), kernel=case.kernels[0])
            assert bool(torch.isfinite(stats[:ns]).all()) and bool(torch.isnan(stats[ns]).all()), (where, "partials beyond the grid's slots")
            (dg, db, co), = _finalizers(call, H, [stats], ns, inp.count, Cc, o.items)
            got["coef"] = co.cpu().numpy()
            Ga = place(inp.a["G"], base)                       # activation derivative and scale only
            d.G, d.coef = Ga.data_ptr(), None
            call("rl_bn_bwd_apply", C.byref(d), kernel=case.kernels[1])
            got["G_act"] = Ga.cpu().numpy()
            d.G, d.coef = G.data_ptr(), co.data_ptr()
            call("rl_bn_bwd_apply", C.byref(d), kernel=case.kernels[1])
        got.update(G=G.cpu().numpy(), dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())
        return got

    def by_ops():
        G = place(inp.a["G"], base)
        y = ops.Lazy(Y, e.B, e.n, e.bstride, Cc, v.get("scale"), v.get("shift"), o.act, B.SLOPE if o.act == B.ACT_LRELU else 0.0,
                     v["mean"], v["invstd"])
        dg, db = filled((Cc,), 7.0), filled((Cc,), 7.0)
        n0 = L.rl_launch_count()
        ops.bn_backward(G, y, dg, db, True)
        assert L.rl_launch_count() == n0 + (1 if small else 3), where
        assert L.rl_last_kernel().decode() == case.kernels[-1], (where, L.rl_last_kernel())
        return dict(G=G.cpu().numpy(), dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())

    got = by_descriptor()
    _note(report, case.family, B.verify_bwd(inp, got, ref), where)
    # ops.bn_backward takes the one-launch form wherever it is supported, the sweeps elsewhere (a base 4 bytes off included)
    if case.misalign == "vectors" or (small and o.count3):
        through_ops = False
    else:
        through_ops = small or not fused_ok or base == 1
    again = by_ops() if through_ops else by_descriptor()
    for k, x in again.items():
        assert _same_bits(x, got[k]), (where, k, "a second run differs", "ops" if through_ops else "descriptor")


def _resid_edge(ops, H, report, case, i, j):
    inp = B.make_bwd(case, i, j)
    ref = B.reference_bwd(inp)
    L = H.lib()
    o, Cc, M = inp.opts, case.C, inp.M
    where = f"{case.id} {inp.edge}"
    call = Calls(H, where)
    t = {k: place(inp.a[k]) for k in inp.a if k != "G"}
    small = case.family == "resid_small"
    assert bool(L.rl_resid_bn_bwd_supported(M, Cc)) and bool(L.rl_resid_bn_bwd_fused_supported(M, Cc)) == (M <= B.SM_ROWS)

    def by_descriptor():
        G, G2 = place(inp.a["G"]), filled((M, Cc), float("nan"))
        d = H.ResidBnBwdDesc()
        d.G, d.G2, d.O, d.slope, d.rows, d.C = G.data_ptr(), G2.data_ptr(), t["O"].data_ptr(), o.resid_slope, M, Cc
        d.Y1, d.scale1, d.mean1, d.invstd1 = (t[k].data_ptr() for k in ("Y1", "scale1", "mean1", "invstd1"))
        d.Y2, d.scale2, d.mean2, d.invstd2 = (t[k].data_ptr() for k in ("Y2", "scale2", "mean2", "invstd2"))
        got = {}
        if small:
            outs = [filled((Cc,), 7.0) for _ in range(4)]
            call("rl_resid_bn_bwd_fused", C.byref(d), *(x.data_ptr() for x in outs), kernel=case.kernels[0])
            got.update(dgamma1=outs[0], dbeta1=outs[1], dgamma2=outs[2], dbeta2=outs[3])
        else:
            ns = B.slots(M)
            assert L.rl_bn_bwd_slots(M) == ns, where
            st = [filled((ns + 1, 2, Cc), float("nan"), torch.float64) for _ in range(2)]
            d.stats1, d.stats2 = st[0].data_ptr(), st[1].data_ptr()
            call("rl_resid_bn_bwd_reduce", C.byref(d), kernel=case.kernels[0])
            for s in st:
                assert bool(torch.isfinite(s[:ns]).all()) and bool(torch.isnan(s[ns]).all()), (where, "partials beyond the grid's slots")
            (dg1, db1, c1), (dg2, db2, c2) = _finalizers(call, H, st, ns, M, Cc, 2)
            d.coef1, d.coef2 = c1.data_ptr(), c2.data_ptr()
            call("rl_resid_bn_bwd_apply", C.byref(d), kernel=case.kernels[1])
            got.update(dgamma1=dg1, dbeta1=db1, dgamma2=dg2, dbeta2=db2, coef1=c1, coef2=c2)
        got.update(G=G, G2=G2)
        return {k: x.cpu().numpy() for k, x in got.items()}

    def by_ops():
        G = place(inp.a["G"])
        y1 = ops.Lazy(t["Y1"], 1, M, M, Cc, t["scale1"], None, 0, 0.0, t["mean1"], t["invstd1"])
        y2 = ops.Lazy(t["Y2"], 1, M, M, Cc, t["scale2"], None, 0, 0.0, t["mean2"], t["invstd2"])
        assert ops.resid_bn_supported(y1, y2)
        outs = [filled((Cc,), 7.0) for _ in range(4)]
        n0 = L.rl_launch_count()
        G2 = ops.resid_bn_backward(G, t["O"], o.resid_slope, y1, y2, *outs)
        assert L.rl_launch_count() == n0 + (1 if small else 3), where
        assert L.rl_last_kernel().decode() == case.kernels[-1], (where, L.rl_last_kernel())
        got = dict(G=G, G2=G2, dgamma1=outs[0], dbeta1=outs[1], dgamma2=outs[2], dbeta2=outs[3])
        return {k: x.cpu().numpy() for k, x in got.items()}

    got = by_descriptor()
    _note(report, case.family, B.verify_bwd(inp, got, ref), where)
    through_ops = small == (M <= B.SM_ROWS)                     # (ops takes the one-launch form up to 2048 rows)
    again = by_ops() if through_ops else by_descriptor()
    for k, x in again.items():
        assert _same_bits(x, got[k]), (where, k, "a second run differs", "ops" if through_ops else "descriptor")


@pytest.mark.parametrize("i", range(len(B.CASES)), ids=[c.id for c in B.CASES])
def test_lattice_row(ops, H, report, i):
    case = B.CASES[i]
    for j in range(len(case.edges)):
        (_resid_edge if case.family.startswith("resid") else _plain_edge)(ops, H, report, case, i, j)


# ---- refusals on real tensors ----------------------------------------------------------------------------------------------------------
def test_one_launch_refusals_launch_nothing(H):
    L = H.lib()
    n0 = L.rl_launch_count()
    G0 = np.random.default_rng(0).standard_normal((2049, 1028)).astype(np.float32)
    G, Y = place(G0), place(G0)
    vec = place(np.ones(1040, dtype=np.float32), 1)
    good = place(np.ones(1040, dtype=np.float32))
    out = [filled((1040,), 7.0) for _ in range(2)]

    def fused(rows, Cc, ld, mean=good, scale=good):
        d = H.BnBwdDesc()
        d.G, d.Y, d.ld, d.bstride, d.B, d.n, d.C = G.data_ptr(), Y.data_ptr(), ld, rows, 1, rows, Cc
        d.scale, d.shift, d.mean, d.invstd = scale.data_ptr(), good.data_ptr(), mean.data_ptr(), good.data_ptr()
        return L.rl_bn_bwd_fused(C.byref(d), rows, out[0].data_ptr(), out[1].data_ptr(), None, H.stream_ptr())

    assert fused(2049, 8, 8) == H.ERR_UNSUPPORTED
    assert fused(64, 6, 8) == H.ERR_UNSUPPORTED
    assert fused(64, 8, 10) == H.ERR_UNSUPPORTED
    assert fused(64, 1028, 1028) == H.ERR_ARGS
    assert fused(64, 8, 8, mean=vec) == H.ERR_ARGS and fused(64, 8, 8, scale=vec) == H.ERR_ARGS
    r = H.ResidBnBwdDesc()
    r.G, r.G2, r.O, r.slope, r.rows, r.C, r.Y1, r.Y2 = G.data_ptr(), Y.data_ptr(), Y.data_ptr(), 0.01, 64, 12, Y.data_ptr(), Y.data_ptr()
    r.scale1 = r.mean1 = r.invstd1 = r.scale2 = r.mean2 = r.invstd2 = good.data_ptr()
    assert L.rl_resid_bn_bwd_fused(C.byref(r), None, None, None, None, H.stream_ptr()) == H.ERR_UNSUPPORTED
    items = (H.BnBwdFinalizeItem * 9)()
    assert L.rl_bn_bwd_finalize_batch(items, 9, H.stream_ptr()) == H.ERR_ARGS
    assert L.rl_launch_count() == n0
    assert np.array_equal(G.cpu().numpy().view(np.int32), G0.view(np.int32)) and bool((out[0] == 7.0).all())


# ---- the forward fold ----------------------------------------------------------------------------------------------------------------------
FOLD_OUT = ("scale", "shift", "save_mean", "save_invstd")


def _fold_state(f, a):
    """The device tensors of one fold: inputs, the buffers it updates in place, its outputs (NaN before the launch)."""
    t = {k: place(a[k]) for k in ("stats", "gamma", "beta", "bias") if k in a}
    for k in ("rmean", "rvar", "nbt", "pivot"):
        if k in a:
            t[k] = place(a[k])
    for k in FOLD_OUT:
        t[k] = filled((f.C,), float("nan"))
    return t


def _fold_args(H, f, t):
    return dict(stats=H.ptr(t.get("stats")), count=f.n, gamma=H.ptr(t.get("gamma")), beta=H.ptr(t.get("beta")), running_mean=H.ptr(t.get("rmean")),
                running_var=H.ptr(t.get("rvar")), num_batches_tracked=H.ptr(t.get("nbt")), scale=t["scale"].data_ptr(), shift=t["shift"].data_ptr(),
                save_mean=t["save_mean"].data_ptr(), save_invstd=t["save_invstd"].data_ptr(), folded_bias=H.ptr(t.get("bias")), nslots=f.nslots,
                C=f.C, training=int(f.training), momentum=float(B.MOMENTUM), eps=float(B.EPS), pivoted=int(f.pivot is not None),
                pivot=H.ptr(t.get("pivot")) if f.training else None)


def _fold_single(H, call, f, t):
    k = _fold_args(H, f, t)
    call("rl_bn_finalize", k["stats"], k["nslots"], k["count"], k["C"], k["gamma"], k["beta"], k["running_mean"], k["running_var"],
         k["num_batches_tracked"], k["momentum"], k["eps"], k["training"], k["scale"], k["shift"], k["save_mean"], k["save_invstd"],
         k["folded_bias"], k["pivoted"], k["pivot"])


def _fold_got(f, a, t):
    got = {k: t[k].cpu().numpy() for k in FOLD_OUT}
    for k in ("rmean", "rvar", "pivot"):
        if k in t:
            got[k] = t[k].cpu().numpy()
    if "nbt" in t:
        got["nbt"] = int(t["nbt"].cpu()[0])
    # what a fold must leave alone: everything in eval, the running buffers' absence is the caller's (nothing to update)
    if not f.training:
        for k in ("rmean", "rvar", "pivot"):
            if k in t:
                assert _same_bits(got[k], a[k]), (f.id, k, "updated in eval mode")
    return got


@pytest.mark.parametrize("k", range(len(B.FOLDS)), ids=[f.id for f in B.FOLDS])
def test_fold_row(H, report, k):
    f = B.FOLDS[k]
    a = B.make_fold(f, k)
    ref = B.reference_fold(f, a)
    call = Calls(H, f.id)
    runs = []
    for _ in range(2):
        t = _fold_state(f, a)
        if not f.running:
            t["nbt"] = place(np.array([5], dtype=np.int64))    # null running buffers: nothing is updated, the counter included
        _fold_single(H, call, f, t)
        got = _fold_got(f, a, t)
        if not f.running:
            assert got.pop("nbt") == 5, (f.id, "num_batches_tracked rose without running buffers")
        runs.append(got)
    _note(report, "fold", B.verify_fold(f, a, runs[0], ref), f.id)
    for name, x in runs[0].items():
        assert x == runs[1][name] if name == "nbt" else _same_bits(x, runs[1][name]), (f.id, name, "a second run differs")


@pytest.mark.parametrize("count", B.FOLD_BATCHES)
def test_fold_batch(H, report, count):
    items = B.batch_items(count)
    args = [B.make_fold(f, 100 * count + k) for k, f in enumerate(items)]
    call = Calls(H, f"fold batch of {count}")
    batch = [_fold_state(f, a) for f, a in zip(items, args)]
    arr = (H.BnFinalizeItem * count)()
    for it, f, t in zip(arr, items, batch):
        for name, val in _fold_args(H, f, t).items():
            setattr(it, name, val)
    call("rl_bn_finalize_batch", arr, count, launches=-(-count // B.BNF_MAX))
    for k, (f, a, t) in enumerate(zip(items, args, batch)):
        got = _fold_got(f, a, t)
        _note(report, "fold", B.verify_fold(f, a, got), f"batch of {count} item {k}")
        one = _fold_state(f, a)
        _fold_single(H, call, f, one)
        alone = _fold_got(f, a, one)
        for name, x in got.items():
            assert x == alone[name] if name == "nbt" else _same_bits(x, alone[name]), (count, k, name, "the batch differs from the single fold")


def test_reduce_slots(H, report):
    for k, (ns, Cc) in enumerate(B.SLOT_CASES):
        x = np.random.default_rng(k).standard_normal((ns, 2, Cc)) * 100.0
        call = Calls(H, f"slots {ns} x {Cc}")
        st, out = place(x), filled((3, Cc), float("nan"), torch.float64)
        call("rl_bn_reduce_slots", st.data_ptr(), ns, Cc, out.data_ptr())
        got = out.cpu().numpy()
        assert np.isnan(got[2]).all()
        ref, bound = B.reference_slots(x)
        _note(report, "reduce_slots", {"totals": B.check(got[:2], ref, bound, call.where)}, call.where)
        # ... and the nslots = 1 finalize the SyncGroup path feeds them to
        co = filled((2 * Cc,), 7.0)
        call("rl_bn_bwd_finalize", out.data_ptr(), 1, 3 * ns, Cc, None, None, co.data_ptr())
        want = ref.reshape(-1) / (3 * ns)
        B.check(co.cpu().numpy(), want, B.stored(want, bound.reshape(-1) / (3 * ns) + B.V * np.abs(want)), call.where + " coef")


def test_backward_finalize_batch_mixed_items(H, report):
    """Eight items of mixed C and slot counts in one launch (grid maxc, early return): each against fp64, bit-equal to the single."""
    spec = [(1, 1), (1024, 255), (5, 256), (64, 257), (3, 1024), (257, 3), (12, 1), (1024, 1024)]
    call = Calls(H, "bwd finalize batch")
    arr = (H.BnBwdFinalizeItem * 8)()
    keep = []
    for k, (Cc, ns) in enumerate(spec):
        x = np.random.default_rng(50 + k).standard_normal((ns, 2, Cc)) * 10.0
        st = place(x)
        dg, db, co = filled((Cc,), 7.0), filled((Cc,), 7.0) if k % 3 else None, filled((2 * Cc,), 7.0)
        it = arr[k]
        it.stats, it.count, it.dgamma, it.dbeta, it.coef, it.nslots, it.C = st.data_ptr(), 16 * ns, dg.data_ptr(), H.ptr(db), co.data_ptr(), ns, Cc
        keep.append((x, st, dg, db, co))
    call("rl_bn_bwd_finalize_batch", arr, 8)
    for k, ((Cc, ns), (x, st, dg, db, co)) in enumerate(zip(spec, keep)):
        ref, bound = B.reference_slots(x)
        where = f"bwd finalize item {k}"
        r = {"dgamma": B.check(dg.cpu().numpy(), ref[1], B.stored(ref[1], bound[1]), where)}
        if db is not None:
            r["dbeta"] = B.check(db.cpu().numpy(), ref[0], B.stored(ref[0], bound[0]), where)
        want = ref.reshape(-1) / (16 * ns)
        r["coef"] = B.check(co.cpu().numpy(), want, B.stored(want, bound.reshape(-1) / (16 * ns) + B.V * np.abs(want)), where)
        _note(report, "bwd_finalize", r, where)
        dg1, co1 = filled((Cc,), 7.0), filled((2 * Cc,), 7.0)
        call("rl_bn_bwd_finalize", st.data_ptr(), ns, 16 * ns, Cc, dg1.data_ptr(), None, co1.data_ptr())
        assert torch.equal(dg1, dg) and torch.equal(co1, co), where
