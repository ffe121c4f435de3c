"""Dropout(fc_end) on the MI355X against a reference that is not the project's own code: every keep bit of rl_dropout_fwd /
rl_dropout_bwd / rl_head_fwd / rl_head_bwd against the numpy Philox twin (oracle/philox_oracle.py, itself pinned to Random123's
known answers by tests/test_philox_cpu.py), the values against plain float32 / float64 arithmetic, and the fused head as a
kernel - loss, counts, input gradient, weight gradients - against a float64 torch autograd through the twin's mask.  Nothing
here is statistical: the mask is a pure function of (seed, key, element index).  p = 0.5 is the one rate at which a swapped
comparison, a 1/p scale or a threshold made from 1 - p cannot be seen, so the cases sit elsewhere."""
import numpy as np
import pytest
import torch

from oracle import philox_oracle as PO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
EPS32 = float(np.finfo(np.float32).eps)
SEED_HI = 5 + (3 << 32)


@pytest.fixture(scope="module")
def ops():
    from randlanet import _ops
    return _ops


def _key(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def _lazy(ops, t, scale=None, shift=None, act=0, slope=0.0):
    rows, C = t.shape
    return ops.Lazy(t, 1, rows, rows, C, scale, shift, act, slope)


def _x(rows, C, seed):
    return np.random.RandomState(seed).standard_normal((rows, C)).astype(np.float32)


def _check_fwd_bwd(ops, rows, C, p, seed=5, key=1, first_row=0):
    """rl_dropout_fwd (no fold) and rl_dropout_bwd on fresh data against the twin: zero pattern exact, kept values bitwise."""
    keep = PO.dropout_keep(seed, key, p, rows, C, first_row)
    scale = PO.dropout_scale(p)
    k = _key(key)
    for which in ("fwd", "bwd"):
        x = _x(rows, C, rows + C + (which == "bwd"))
        t = torch.from_numpy(x).to(DEV)
        if which == "fwd":
            out = ops.dropout_fwd(_lazy(ops, t), k, seed, p, first_row)
            assert torch.equal(t.cpu(), torch.from_numpy(x))            # the source is left alone
        else:
            ops.dropout_bwd(t, k, seed, p, first_row)                   # in place
            out = t
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got == 0.0, ~keep, err_msg=f"{which}: zero pattern")      # (randn draws no exact 0)
        want = np.where(keep, x * scale, np.float32(0))
        assert want.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"{which}: values")
    return keep


@pytest.mark.parametrize("p", [0.0, 0.1, 0.3, 0.5, 0.9])
@pytest.mark.parametrize("rows,C", [(r, c) for r in (1, 257, 1031) for c in (4, 32, 64)])
def test_dropout_kernels_match_the_twin(ops, rows, C, p):
    keep = _check_fwd_bwd(ops, rows, C, p)
    if p == 0.0:
        assert keep.all()


def test_dropout_past_the_grid_cap(ops):
    """grid_for caps a launch at 4096 workgroups of 256 lanes = 2^20 quads per grid-stride trip; 1031 x 64 / 4 = 16496 quads
    stay far below it.  65537 rows of 64: 2^20 + 16 quads - the first 16 lanes of workgroup 0 take a second trip."""
    rows, C = 65537, 64
    assert rows * C // 4 > 4096 * 256
    _check_fwd_bwd(ops, rows, C, 0.3)


@pytest.mark.parametrize("act", ["ACT_NONE", "ACT_RELU", "ACT_LRELU"])
@pytest.mark.parametrize("p", [0.1, 0.9])
@pytest.mark.parametrize("rows,C", [(257, 4), (1031, 32), (257, 64)])
def test_dropout_fwd_with_the_lazy_fold(ops, rows, C, p, act):
    """The producer's folded BatchNorm + activation applied on load, then Dropout: against act(x * scale + shift) in float64
    times the float32 Dropout scale.  Per element the kernel rounds the affine once (fused) or twice (product, sum), the
    slope product and the final multiply - each at most eps32 / 2 of a value bounded by (|x * scale| + |shift|) * dscale:
    at most 2 eps32 of it; asserted at 4 eps32 (derived, not measured)."""
    from randlanet import _hip as H
    assert {n for n in dir(H) if n.startswith("ACT_")} == {"ACT_NONE", "ACT_RELU", "ACT_LRELU"}     # every ACT_* there is
    rs = np.random.RandomState(rows * C)
    x = rs.standard_normal((rows, C)).astype(np.float32)
    sc = rs.uniform(0.5, 1.5, C).astype(np.float32) * np.where(rs.uniform(size=C) < 0.25, -1, 1).astype(np.float32)
    sh = rs.standard_normal(C).astype(np.float32)
    slope = 0.2
    keep = PO.dropout_keep(SEED_HI, 9, p, rows, C)
    t = torch.from_numpy(x).to(DEV)
    lz = _lazy(ops, t, torch.from_numpy(sc).to(DEV), torch.from_numpy(sh).to(DEV), getattr(H, act), slope)
    got = ops.dropout_fwd(lz, _key(9), SEED_HI, p).cpu().numpy().astype(np.float64)
    aff = x.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)
    if act == "ACT_RELU":
        aff = np.maximum(aff, 0.0)
    elif act == "ACT_LRELU":
        aff = np.where(aff > 0, aff, aff * float(np.float32(slope)))
    dscale = float(PO.dropout_scale(p))
    want = np.where(keep, aff * dscale, 0.0)
    bound = 4 * EPS32 * (np.abs(x.astype(np.float64) * sc) + np.abs(sh.astype(np.float64))) * dscale
    ratio = float((np.abs(got - want) / bound).max())
    print(f"[lazy fold] {rows} x {C}, p = {p}, {act}: worst |error| / bound = {ratio:.3f}")
    np.testing.assert_array_equal(got[~keep], 0.0)
    assert ratio <= 1.0, ratio
    if act == "ACT_NONE":
        np.testing.assert_array_equal(got == 0.0, ~keep)
    else:
        assert (got[keep & (aff > 1e-3)] != 0.0).all()


# ------------------------------------------------------------------------------------------------ the counter
def _mask_of(ops, rows, C, p, seed, key_t, first_row=0):
    """The keep pattern the kernel draws, read off a tensor of ones."""
    out = ops.dropout_fwd(_lazy(ops, torch.ones((rows, C), device=DEV)), key_t, seed, p, first_row)
    return out.cpu().numpy() != 0.0


def test_first_row_offsets_the_counter(ops):
    rows, C, p = 1031, 32, 0.3
    whole = _mask_of(ops, rows, C, p, 5, _key(1))
    np.testing.assert_array_equal(whole, PO.dropout_keep(5, 1, p, rows, C))
    part = _mask_of(ops, rows - 700, C, p, 5, _key(1), first_row=700)
    np.testing.assert_array_equal(part, whole[700:])
    assert (part != whole[:rows - 700]).any()
    _check_fwd_bwd(ops, rows - 700, C, p, first_row=700)


def test_high_counter_seed_and_key_words(ops):
    """Each 64-bit input of the generator with a non-zero high word: equal to the twin, different from the low word alone."""
    rows, C, p = 257, 32, 0.3
    base = _mask_of(ops, rows, C, p, 5, _key(1))
    np.testing.assert_array_equal(base, PO.dropout_keep(5, 1, p, rows, C))
    # first_row = 2^31 at 32 channels: quad index 2^34
    far = _check_fwd_bwd(ops, rows, C, p, first_row=2 ** 31)
    assert (far != base).any()
    np.testing.assert_array_equal(_mask_of(ops, rows, C, p, 5, _key(1), first_row=2 ** 31), far)
    # the seed's high word
    hi_seed = _check_fwd_bwd(ops, rows, C, p, seed=SEED_HI)
    assert (hi_seed != base).any()
    # the key's high word (a key tensor written by hand: rl_dropout_tick counts from 1)
    for key in (1 + (1 << 32), 1 + (5 << 40)):
        hi_key = _check_fwd_bwd(ops, rows, C, p, key=key)
        assert (hi_key != base).any()


def _threshold_hits(seed, key, rows, first_row=0):
    """Elements of a (rows, 32) tensor whose Philox word lies in [1, 2^24): each such word w is the threshold of the float32
    rate p = w / 2^32 exactly (tests/test_philox_cpu.py), the one place where `>=` and `>` part."""
    gq = np.uint64(first_row * 8) + np.arange(rows * 8, dtype=np.uint64)
    words = np.stack(PO.philox4x32_10((gq & PO.M32, gq >> np.uint64(32), key & 0xFFFFFFFF, key >> 32),
                                      (seed & 0xFFFFFFFF, seed >> 32)), axis=-1).reshape(-1)
    hits = np.flatnonzero((words < (1 << 24)) & (words > 0))
    assert len(hits) >= 3
    return [(int(e), int(words[e])) for e in hits[:3]]


def test_a_word_equal_to_the_threshold_is_kept(ops):
    rows, C = 257, 32
    for e, w in _threshold_hits(5, 1, rows):
        p = float(np.float32(w / 2.0 ** 32))
        assert PO.dropout_threshold(p) == w
        keep = _check_fwd_bwd(ops, rows, C, p)
        assert keep.reshape(-1)[e]
        p1 = float(np.float32((w + 1) / 2.0 ** 32))
        assert not _check_fwd_bwd(ops, rows, C, p1).reshape(-1)[e]


def test_dropout_tick_counts_and_keys_the_masks(ops):
    rows, C, p = 257, 32, 0.3
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    masks = []
    for want in (1, 2, 3):
        key = ops.dropout_tick(counter)
        assert key.dtype == torch.int64 and int(key) == want
        masks.append(_mask_of(ops, rows, C, p, 5, key))
        np.testing.assert_array_equal(masks[-1], PO.dropout_keep(5, want, p, rows, C))
    assert int(counter) == 3
    assert (masks[0] != masks[1]).any() and (masks[1] != masks[2]).any() and (masks[0] != masks[2]).any()


def test_dropped_non_finite_values_become_zero(ops):
    """keep ? v * scale : 0, not v * keep: an infinity or a NaN at a dropped position leaves a plain 0.0 (forward and backward)."""
    rows, C, p = 257, 32, 0.3
    keep = PO.dropout_keep(5, 1, p, rows, C)
    dropped = np.argwhere(~keep)
    kept = np.argwhere(keep)
    (r0, c0), (r1, c1), (r2, c2) = dropped[3], dropped[len(dropped) // 2], dropped[-1]
    (r3, c3) = kept[7]
    x = _x(rows, C, 1)
    x[r0, c0], x[r1, c1], x[r2, c2], x[r3, c3] = np.inf, np.nan, -np.inf, np.inf
    want = np.where(keep, x * PO.dropout_scale(p), np.float32(0))
    assert want[r0, c0] == 0 and want[r1, c1] == 0 and want[r2, c2] == 0 and want[r3, c3] == np.inf
    t = torch.from_numpy(x).to(DEV)
    fwd = ops.dropout_fwd(_lazy(ops, t), _key(1), 5, p).cpu().numpy()
    ops.dropout_bwd(t, _key(1), 5, p)
    for got in (fwd, t.cpu().numpy()):
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))       # (+0.0 exactly, bit for bit)


def test_scale_mask_matches_where(ops):
    rows, C = 1031, 32
    rs = np.random.RandomState(3)
    x = rs.standard_normal((rows, C)).astype(np.float32)
    mask = (rs.uniform(size=(rows, C)) < 0.7).astype(np.uint8)
    scale = 1.0 / 0.7
    t = torch.from_numpy(x).to(DEV)
    ops.scale_mask(t, torch.from_numpy(mask).to(DEV), scale)
    want = np.where(mask != 0, x * np.float32(scale), np.float32(0))
    np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the fused head
@pytest.mark.parametrize("C", [3, 13])
def test_head_keeps_a_word_equal_to_the_threshold(ops, C):
    """The same edge in the fused head's own copy of the generator (register and MFMA forward kernels): Head.mask."""
    from randlanet import _hip as H
    B, N, key, first_row = 1, 517, 3, 4096
    rs = np.random.RandomState(C)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    x = ops.Lazy(dev(rs.standard_normal((N, 32)).astype(np.float32)), B, N, N, 32)
    W, bias = dev(rs.standard_normal((C, 32)).astype(np.float32)), dev(rs.standard_normal(C).astype(np.float32))
    perm, labels = dev(rs.permutation(N)), dev(rs.randint(0, C, size=(B, N)).astype(np.int64))
    for e, w in _threshold_hits(SEED_HI, key, N, first_row):
        for thr, kept in ((w, True), (w + 1, False)):
            p = float(np.float32(thr / 2.0 ** 32))
            head = ops.Head(labels, 0, 0.0, 0.0, True, torch.zeros(1 + 4 * C, dtype=torch.float64, device=DEV))
            ops.head_fwd(x, W, bias, perm, head, (_key(key), SEED_HI, p, first_row))
            keep = PO.dropout_keep(SEED_HI, key, p, N, 32, first_row)
            assert bool(keep.reshape(-1)[e]) == kept
            np.testing.assert_array_equal(head.mask.cpu().numpy().view(np.uint32), PO.keep_words(keep))


HEAD_CASES = [      # C: 2 / 3 / 8 -> the register kernels <2> / <4> / <8>; 13 -> MFMA <16>; 20, 32 -> MFMA <32>
    ("cross_entropy", 2, 0.3, 0), ("dice", 3, 0.8, 4096), ("focal_tversky", 8, 0.3, 4096), ("cross_entropy", 8, 0.8, 0),
    ("cross_entropy", 13, 0.8, 4096), ("focal_tversky", 13, 0.3, 0), ("dice", 20, 0.3, 0), ("focal_tversky", 32, 0.8, 0),
    ("dice", 32, 0.3, 4096),
    ("cross_entropy", 3, 0.3, 2 ** 31), ("dice", 13, 0.8, 2 ** 31),       # quad index 2^34: the head's own high counter word
]


@pytest.mark.parametrize("loss_name,C,p,first_row", HEAD_CASES)
def test_head_kernels_match_fp64_autograd(ops, loss_name, C, p, first_row):
    """rl_head_fwd / rl_head_bwd as kernels on a synthetic lazy tensor (2 x 517 = 1034 rows: five workgroups, a ragged last
    trip), seed above 2^32: Head.mask against the twin exactly; loss, counts, G and the reduced dW / db against a float64
    autograd of  z = relu(x * scale + shift), d = z * keep * dscale, logits = d W^T + b, un-permuted, loss_by_name.
    Tolerances: the ones test_fused_head_equals_the_separate_launches holds this head to - counts equal, loss rtol 2e-6,
    gradients 2e-4 of the tensor's largest entry (measured against fp64: loss <= 1.2e-8 relative, G / dW / db <= 3.7e-7 of
    their scale - the fp32 head needs no more).  Then rl_head_bwd once more WITHOUT the stored mask (the branch that
    regenerates the keep bits): G and the slab bitwise equal."""
    from oracle.loss_metrics_oracle import loss_by_name
    from randlanet import _hip as H
    B, N, key = 2, 517, 3
    rows = B * N
    rs = np.random.RandomState(100 * C + first_row % 7 + (first_row >> 31))
    X = rs.standard_normal((rows, 32)).astype(np.float32)
    sc = rs.uniform(0.5, 1.5, 32).astype(np.float32)
    sh = (0.5 * rs.standard_normal(32)).astype(np.float32)
    W = (0.3 * rs.standard_normal((C, 32))).astype(np.float32)
    bias = (0.3 * rs.standard_normal(C)).astype(np.float32)
    perm = rs.permutation(N)
    labels = rs.randint(0, C, size=(B, N)).astype(np.int64)
    kind, alpha, gamma = ops.LOSS_KINDS[loss_name]

    dev = lambda a: torch.from_numpy(a).to(DEV)
    x = ops.Lazy(dev(X), B, N, N, 32, dev(sc), dev(sh), H.ACT_RELU, 0.0)        # mean = None: no BatchNorm-backward sums
    Wd, bd, pd = dev(W), dev(bias), dev(perm)
    head = ops.Head(dev(labels), kind, alpha, gamma, True, torch.zeros(1 + 4 * C, dtype=torch.float64, device=DEV))
    drop = (_key(key), SEED_HI, p, first_row)
    ops.head_fwd(x, Wd, bd, pd, head, drop)
    keep = PO.dropout_keep(SEED_HI, key, p, rows, 32, first_row)
    assert head.mask is not None and head.mask.numel() == rows
    np.testing.assert_array_equal(head.mask.cpu().numpy().view(np.uint32), PO.keep_words(keep))

    def backward():
        dW = torch.zeros((C, 32), device=DEV)
        db = torch.zeros(C, device=DEV)
        pending = []
        G, pre = ops.head_bwd(x, Wd, bd, pd, head, drop, dW, db, pending)
        assert pre is None
        slab = pending[0][1].clone()
        ops.wgrad_flush(pending)                  # rl_wgrad_reduce_batch, as the training step does
        return G.cpu(), slab.cpu(), dW.cpu(), db.cpu()
    G, slab, dW, db = backward()
    stored = head.mask
    head.mask = None
    G2, slab2, dW2, db2 = backward()
    head.mask = stored
    assert torch.equal(G, G2) and torch.equal(slab, slab2) and torch.equal(dW, dW2) and torch.equal(db, db2)
    out = head.out.cpu().numpy()

    # float64 reference
    t64 = lambda a: torch.from_numpy(a.astype(np.float64))
    z = torch.relu(t64(X) * t64(sc) + t64(sh)).requires_grad_(True)
    W64, b64 = t64(W).requires_grad_(True), t64(bias).requires_grad_(True)
    d = z * t64(keep) * float(PO.dropout_scale(p))
    lp = d @ W64.T + b64                                                       # (rows, C), permuted order
    L = torch.zeros((B, N, C), dtype=torch.float64)
    L = L.index_copy(1, torch.from_numpy(perm), lp.view(B, N, C))              # row r of cloud b is point perm[r]
    logits = L.permute(0, 2, 1)
    loss = loss_by_name(loss_name, logits, torch.from_numpy(labels))
    loss.backward()
    pred = logits.detach().argmax(1).numpy()
    inter = np.array([((pred == c) & (labels == c)).sum() for c in range(C)], dtype=np.float64)
    lab = np.array([(labels == c).sum() for c in range(C)], dtype=np.float64)
    prd = np.array([(pred == c).sum() for c in range(C)], dtype=np.float64)
    psum = torch.softmax(logits.detach(), 1).sum((0, 2)).numpy()

    errs = {n: float((g.double() - r).abs().max()) / float(r.abs().max())
            for n, g, r in (("G", G, z.grad), ("dW", dW, W64.grad), ("db", db, b64.grad))}
    print(f"[head] {loss_name} C={C} p={p} first_row={first_row}: loss {out[0]:.9f} vs {float(loss):.9f} "
          f"(rel {abs(out[0] - float(loss)) / abs(float(loss)):.1e}), gradient errors / scale "
          + ", ".join(f"{n} {e:.1e}" for n, e in errs.items()))
    np.testing.assert_allclose(out[0], float(loss), rtol=2e-6, atol=1e-7)
    np.testing.assert_array_equal(out[1:1 + 3 * C].reshape(3, C), np.stack([inter, lab, prd]))
    np.testing.assert_allclose(out[1 + 3 * C:], psum, rtol=1e-5)
    for n, e in errs.items():
        assert e < 2e-4, (n, e)
    # the gradient is zero exactly where the mask drops
    np.testing.assert_array_equal(G.numpy()[~keep], 0.0)
