"""The gather path's kernels on the MI355X, one case per row of tests/gather_lattice.py.

rl_csr_build: every row through the C ABI with a workspace of exactly rl_csr_workspace_bytes inside 256-byte bands of a sentinel,
offsets and entries in guarded buffers likewise; integer equality with the stable-argsort reference, silence around all three, the
kernel rl_last_kernel names is the restated plan's, and a second build (through ops.csr_build) has the same bits.
rl_segment_sum_rows: through the descriptor on the REFERENCE offsets / entries (a CSR defect cannot steer its reads; one row chains
the device's CSR as the engine does): every element inside the fp64 bound, equal by value to the fp32 sum in segment order, silence
outside the addressed block, a second run bit-equal.
rl_copy_rows / rl_copy_rows_pair / rl_scatter_add_rows: through the descriptor; the fp64 bound per element, the fp32 expression by
value, silence outside; the pair against two single calls bit for bit.
Every index is asserted in range on the host before a launch (the "dropped" graphs of table 1 excepted: the kernels' guard is what
they test).  The largest error / bound per kernel family and option, and the file's wall time, are printed when the module is done.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import gather_lattice as G

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
        print(f"[gather lattice] {fam:<34} max error / bound {ratio:.3f}  ({where})")
    print(f"[gather lattice] wall time {time.perf_counter() - t0:.1f} s")


def _note(report, fam, ratio, where):
    if ratio >= report.get(fam, (-1.0, ""))[0]:
        report[fam] = (ratio, where)


def up(x: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    assert t.data_ptr() % 256 == 0
    return t


def body_ptr(t: torch.Tensor) -> int:
    """The address behind the front guard band of an uploaded guarded buffer."""
    return t.data_ptr() + 4 * G.GUARD


def body_view(t: torch.Tensor, rows: int, ld: int) -> torch.Tensor:
    """The same storage as a (rows, ld) tensor, for the Python wrappers."""
    return t[G.GUARD:G.GUARD + rows * ld].view(rows, ld)


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- table 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(G.CSR_ROWS)), ids=[r.id for r in G.CSR_ROWS])
def test_csr_row(ops, H, i):
    row, data = G.CSR_ROWS[i], G.make_csr(i)
    L = H.lib()
    idx_t = []
    for g, idx, off, ent, kept in data:
        if not g.dropped:
            assert idx.min() >= 0 and idx.max() < g.n_dst, row.id
        idx_t.append(up(idx))
    t0, first = 0, []
    for chunk in G.csr_chunks(row):
        part, part_idx = data[t0:t0 + len(chunk)], idx_t[t0:t0 + len(chunk)]
        t0 += len(chunk)
        plan = G.csr_plan(row.B, chunk)
        arr = (H.CsrTask * len(chunk))()
        outs = []
        for t, (g, idx, off, ent, kept), it in zip(arr, part, part_idx):
            ob, eb = up(G.guarded(row.B * (g.n_dst + 1))), up(G.guarded(row.B * g.per))
            t.idx, t.n_src, t.k, t.n_dst, t.offsets, t.entries = it.data_ptr(), g.n_src, g.k, g.n_dst, body_ptr(ob), body_ptr(eb)
            outs.append((ob, eb))
        nbytes = L.rl_csr_workspace_bytes(arr, len(chunk), row.B)
        assert nbytes == plan["bytes"] and nbytes % 256 == 0, row.id
        ws = up(G.guarded(nbytes // 4))
        rc = L.rl_csr_build(arr, len(chunk), row.B, body_ptr(ws), nbytes, H.stream_ptr())
        assert rc == 0, (row.id, L.rl_last_error())
        assert L.rl_last_kernel().decode() == plan["last_kernel"], (row.id, L.rl_last_kernel())
        torch.cuda.synchronize()
        assert G.silent(ws.cpu().numpy()), f"{row.id}: wrote outside the workspace of rl_csr_workspace_bytes"
        for n, ((g, idx, off, ent, kept), (ob, eb)) in enumerate(zip(part, outs)):
            o, e = ob.cpu().numpy(), eb.cpu().numpy()
            G.verify_csr(g, off, ent, kept, o, e, what=f"{row.id} task {t0 - len(chunk) + n} {g}")
            first.append((o, e))
    again = ops.csr_build([(it, g.n_dst) for it, (g, *_) in zip(idx_t, data)])
    assert len(again) == len(data)
    for n, (csr, (g, idx, off, ent, kept), (o, e)) in enumerate(zip(again, data, first)):
        assert np.array_equal(csr.offsets.cpu().numpy().reshape(-1), o[G.GUARD:-G.GUARD]), (row.id, n, "a second build's offsets differ")
        e1, e0 = csr.entries.cpu().numpy(), e[G.GUARD:-G.GUARD].reshape(row.B, g.per)
        for b in range(row.B):
            assert np.array_equal(e1[b, :kept[b]], e0[b, :kept[b]]), (row.id, n, b, "a second build's entries differ")


# ---- table 2 ------------------------------------------------------------------------------------------------------------------------
def _seg_family(r, d):
    return ("segment_sum " + ("vec" if d["vec"] else "scalar") + (" bf16" if r.bf16 else "") + (" chunked" if d["chunk"] else "") +
            (" capped" if d["capped"] else "") + (" acc" if r.acc else ""))


@pytest.mark.parametrize("i", range(len(G.SEG_ROWS)), ids=[r.id for r in G.SEG_ROWS])
def test_segment_sum_row(ops, H, report, i):
    s = G.make_seg(i)
    r, L = s.row, H.lib()
    G.seg_indices_in_range(s)
    d = G.seg_dispatch(r)
    assert not d["refused"]
    x_t = up(G.bf16_bits(s.x)).view(torch.bfloat16) if r.bf16 else up(s.x)
    assert tuple(x_t.shape) == (r.src_rows, r.lds)
    if r.chain:
        (csr,) = ops.csr_build([(up(s.idx), r.g.n_dst)])
        off_t, ent_t = csr.offsets, csr.entries
        assert np.array_equal(off_t.cpu().numpy(), s.off) and np.array_equal(ent_t.cpu().numpy(), s.ent), "the device's CSR is not the reference"
    else:
        off_t, ent_t = up(s.off), up(s.ent)
    ref = G.reference_seg(s)
    emu = G.emulate_seg(s)
    runs = []
    for through_ops in (False, r.ldd_pad == 0):        # the wrapper cannot say ldd > C: those rows run twice through the descriptor
        dst = up(G.seg_initial(s))
        if through_ops:
            csr = ops.Csr(off_t, ent_t, r.B, r.g.n_src, r.g.k, r.g.n_dst)
            ops.segment_sum_rows(x_t, (r.col0, r.C), r.src_bstride, csr, body_view(dst, r.dst_rows, r.ldd), r.dst_bstride, accumulate=r.acc)
            assert L.rl_last_kernel().decode() == d["kernel"], (r.id, L.rl_last_kernel())
            runs.append(dst.cpu().numpy())
            continue
        desc = H.SegsumDesc()
        desc.src, desc.lds, desc.src_bstride = x_t.data_ptr() + r.col0 * x_t.element_size(), r.lds, r.src_bstride
        desc.dst, desc.ldd, desc.dst_bstride = body_ptr(dst), r.ldd, r.dst_bstride
        desc.offsets, desc.entries, desc.entries_per_cloud = off_t.data_ptr(), ent_t.data_ptr(), r.g.per
        desc.B, desc.n_dst, desc.C, desc.accumulate, desc.src_bf16 = r.B, r.g.n_dst, r.C, int(r.acc), int(r.bf16)
        rc = L.rl_segment_sum_rows(C.byref(desc), H.stream_ptr())
        assert rc == 0, (r.id, L.rl_last_error())
        assert L.rl_last_kernel().decode() == d["kernel"], (r.id, L.rl_last_kernel())
        runs.append(dst.cpu().numpy())
    _note(report, _seg_family(r, d), G.verify_seg(s, runs[0], ref=ref, emu=emu), r.id)
    assert _same_bits(runs[0], runs[1]), (r.id, "a second run differs")


# ---- table 3 ------------------------------------------------------------------------------------------------------------------------
def _copy_launch_args(H, c):
    """(descriptor, destination tensor, everything that must stay alive) of one copy."""
    r = c.row
    x_t, dst = up(c.x), up(G.copy_initial(c))
    keep = [x_t, dst]
    d = H.RowsDesc()
    d.src, d.lds, d.src_bstride = x_t.data_ptr() + 4 * r.c0s, r.lds, r.src_bstride
    d.dst, d.ldd = body_ptr(dst) + 4 * r.c0d, r.ldd
    d.rows, d.rows_per_batch, d.C = r.rows, r.rows_per_batch, r.C
    if c.index is not None:
        G.copy_src_rows(c)                                  # asserts the range
        it = up(c.index.astype(np.int32 if r.index.startswith("i32") else np.int64))
        keep.append(it)
        if r.index.startswith("i32"):
            d.index32 = it.data_ptr()
        else:
            d.index64 = it.data_ptr()
    d.index_shared, d.accumulate = int(r.index.endswith("s")), int(r.acc)
    if r.lazy != "none":
        sc, sh = torch.zeros(r.C + 8, device=DEV), up(c.shift)
        sc[r.scale_off:r.scale_off + r.C] = torch.from_numpy(c.scale).to(DEV)
        keep += [sc, sh]
        d.scale, d.shift, d.act, d.slope = sc.data_ptr() + 4 * r.scale_off, sh.data_ptr(), r.act, G.SLOPE if r.lazy == "lrelu" else 0.0
    return d, dst, keep


def _copy_family(r, disp):
    return f"copy_rows<{disp['vec']}, {disp['itype']}>" + ("" if r.lazy == "none" else f" {r.lazy}") + (" acc" if r.acc else "")


@pytest.mark.parametrize("i", range(len(G.COPY_ROWS)), ids=[r.id for r in G.COPY_ROWS])
def test_copy_row(ops, H, report, i):
    r, L = G.COPY_ROWS[i], H.lib()
    c = G.make_copy(r, G.seed(3, i))
    runs = []
    for second in ((False,) if r.big else (False, True)):
        d, dst, keep = _copy_launch_args(H, c)
        if second and (r.lazy == "none" or r.c0s == 0):      # the wrapper takes a lazy source from column 0 only
            lz = None
            if r.lazy != "none":
                sc, sh = keep[-2:]
                lz = ops.Lazy(keep[0], r.B, r.n, r.src_bstride, r.C, sc[r.scale_off:r.scale_off + r.C], sh, r.act, G.SLOPE if r.lazy == "lrelu" else 0.0)
            ops.copy_rows(keep[0], (r.c0s, r.C), r.src_bstride, body_view(dst, r.dst_rows, r.ldd), (r.c0d, r.C), r.rows, r.rows_per_batch,
                          index=None if c.index is None else keep[2], index_shared=r.index.endswith("s"), accumulate=r.acc, lazy=lz)
        else:
            rc = L.rl_copy_rows(C.byref(d), H.stream_ptr())
            assert rc == 0, (r.id, L.rl_last_error())
        assert L.rl_last_kernel().decode() == "copy_rows_kernel"
        runs.append(dst.cpu().numpy())
    _note(report, _copy_family(r, G.copy_dispatch(r)), G.verify_copy(c, runs[0]), r.id)
    assert _same_bits(runs[0], runs[-1]), (r.id, "a second run differs")


@pytest.mark.parametrize("k", range(len(G.PAIR_ROWS)), ids=[f"{a.id}+{b.id}" for a, b, _ in G.PAIR_ROWS])
def test_copy_pair(H, report, k):
    ra, rb, kernel = G.PAIR_ROWS[k]
    L = H.lib()
    assert (G.pair_eligible(ra) and G.pair_eligible(rb)) == (kernel == "copy_rows_pair_kernel")
    ca, cb = G.make_copy(ra, G.seed(5, 2 * k)), G.make_copy(rb, G.seed(5, 2 * k + 1))
    (da, dsta, ka), (db, dstb, kb) = _copy_launch_args(H, ca), _copy_launch_args(H, cb)
    n0 = L.rl_launch_count()
    rc = L.rl_copy_rows_pair(C.byref(da), C.byref(db), H.stream_ptr())
    assert rc == 0, L.rl_last_error()
    assert L.rl_last_kernel().decode() == kernel and L.rl_launch_count() == n0 + (1 if kernel == "copy_rows_pair_kernel" else 2)
    pa, pb = dsta.cpu().numpy(), dstb.cpu().numpy()
    _note(report, "copy_rows_pair" if kernel.startswith("copy_rows_pair") else "copy_rows_pair fallback",
          max(G.verify_copy(ca, pa), G.verify_copy(cb, pb)), f"{ra.id}+{rb.id}")
    for c, paired in ((ca, pa), (cb, pb)):
        d, dst, keep = _copy_launch_args(H, c)
        assert L.rl_copy_rows(C.byref(d), H.stream_ptr()) == 0
        assert _same_bits(dst.cpu().numpy(), paired), (c.row.id, "the pair differs from the single call")


@pytest.mark.parametrize("i", range(len(G.SCAT_ROWS)), ids=[r.id for r in G.SCAT_ROWS])
def test_scatter_add_row(H, report, monkeypatch, i):
    monkeypatch.setenv("RL_ALLOW_FLOAT_ATOMICS", "1")
    r, x, index = G.make_scat(i)
    L = H.lib()
    G.scat_dst_rows(r, index)                                # asserts the range
    x_t, dst = up(x), up(G.scat_initial(r))
    it = up(index.astype(np.int32 if r.index.startswith("i32") else np.int64))
    d = H.RowsDesc()
    d.src, d.lds, d.src_bstride = x_t.data_ptr() + 4 * r.c0s, r.lds, r.dst_bstride
    d.dst, d.ldd = body_ptr(dst), r.ldd
    d.rows, d.rows_per_batch, d.C = r.rows, r.rows_per_batch, r.C
    if r.index.startswith("i32"):
        d.index32 = it.data_ptr()
    else:
        d.index64 = it.data_ptr()
    d.index_shared = int(r.index.endswith("s"))
    rc = L.rl_scatter_add_rows(C.byref(d), H.stream_ptr())
    assert rc == 0, (r.id, L.rl_last_error())
    assert L.rl_last_kernel().decode() == "scatter_add_rows_kernel"
    _note(report, "scatter_add_rows" + ("<int64_t>" if r.wide else "<uint32_t>"), G.verify_scat(r, x, index, dst.cpu().numpy()), r.id)
