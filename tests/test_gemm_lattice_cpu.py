"""The GEMM / weight-gradient lattice without a GPU: the case table of tests/gemm_lattice.py against the planner, and its checker
against mutants of a CPU emulation.

Table against planner: for every row at every M edge (and option rotation), rl_gemm_plan / rl_wgrad_plan2 on a descriptor of
16-byte-aligned dummy pointers (compared, never dereferenced; nothing is launched) answers exactly the row's expected plan, and
the instantiations the table reaches are the ones the module writes out.  A planner change that reroutes a shape fails here.
(A host without a GPU plans for 256 compute units, the MI355X's count; the one row that depends on it computes its M from it.)

The checker has teeth: a faithful fp32 / bf16x3 / bf16 emulation of the product passes the elementwise bound and each mutant -
one k term dropped, the last row computed from the row before, two output columns swapped, the bias added twice, `accumulate`
ignored, a_lo.w_hi missing (bf16x3), the operand rounded to bf16 (fp32), a leaky slope applied as ReLU - is rejected, at every
K <= 128 tried.  The bound is a worst case that grows as K while a correct kernel's error grows as sqrt(K): at K = 512 / 1024 it has
lost that power (the last test measures how much), and the small-K rows of each kernel family carry the burden.
"""
import pytest
import torch

import gemm_lattice as G


@pytest.fixture(scope="module")
def HL():
    from randlanet import _hip as H
    L = H.lib()
    mode0 = L.rl_get_wide_gemm()
    yield H, L
    G.restore_settings(L, mode0)


def _plan(H, L, case, i, j, M):
    inp = G.make_inputs(case, i, j, M)
    if case.op == "gemm":
        return H.gemm_plan(G.gemm_desc_dummy(H, L, inp)), inp
    return H.wgrad_plan(G.wgrad_desc_dummy(H, L, inp)), inp


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=[c.id for c in G.CASES])
def test_table_row_is_what_the_planner_plans(HL, i):
    H, L = HL
    case = G.CASES[i]
    mode0 = L.rl_get_wide_gemm()
    try:
        G.apply_settings(L, case)
        for j, M in enumerate(G.case_Ms(case)):
            plan, _ = _plan(H, L, case, i, j, M)
            assert plan["rc"] == 0, (case.id, M, L.rl_last_error())
            G.plan_matches(case, plan, M)
            if case.id == "wgemm2_overcap":
                ny = -(-case.N // case.tile[1])
                cap = G.persistent_rows(256, ny)
                assert -(-M // case.tile[0]) > cap and plan["grid"][0] == 8 * (-(-cap // 8)) * ny, (M, cap, plan)
    finally:
        G.restore_settings(L, mode0)


def test_the_table_reaches_the_written_out_variants_and_every_option_meets_every_row():
    gemm = [c for c in G.CASES if c.op == "gemm"]
    wgrad = [c for c in G.CASES if c.op == "wgrad"]
    assert {c.variant for c in gemm} == G.GEMM_VARIANTS
    assert {c.kernel for c in gemm} == G.GEMM_KERNELS
    assert {c.variant for c in wgrad} == G.WGRAD_VARIANTS
    assert {c.reduce_cols for c in gemm} == {0, 16}
    for c in G.CASES:
        assert all(M == G.OVERCAP or M >= 1 for M in c.Ms) and (len(c.Ms) >= 4 or c.Ms == (G.OVERCAP,))
        assert not (c.planes and c.mode == "fp32"), "pre-split planes do not exist in the fp32 mode"
    # the rotation: over the M edges of ANY row every option takes each of its values
    for i in range(len(G.CASES)):
        seen = [G.options(i, j) for j in range(4)]
        for name, values in (("w_n_contig", {False, True}), ("bias", {False, True}), ("accumulate", {False, True}),
                             ("lazy", {None, 0, 1, 2}), ("a_bstride", {False, True}), ("y_bstride", {False, True}),
                             ("pivot", {False, True})):
            assert {getattr(o, name) for o in seen} == values, (i, name)
        assert {G.options(i, j).dbias for j in range(5)} == {False, True}


def test_planner_refusals_on_the_lattice(HL):
    """What the table leaves out by construction is refused, not rerouted: a concat-gather operand on the wide kernel whose rows
    per cloud are no multiple of 16, bf16 rows in the fp32 mode, and the split-K reducer <64> that no shape reaches."""
    H, L = HL
    mode0 = L.rl_get_wide_gemm()
    try:
        i, case = next((i, c) for i, c in enumerate(G.CASES) if c.id == "wgemm2cat_64x64_bf16x3")
        G.apply_settings(L, case)
        for M in (127, 129, 385, 8):
            plan, _ = _plan(H, L, case, i, 0, M)
            assert plan["rc"] == H.ERR_UNSUPPORTED and b"concat-gather" in L.rl_last_error(), (M, plan)
        i, case = next((i, c) for i, c in enumerate(G.CASES) if c.id == "pwgrad128w_bf16rows")
        G.apply_settings(L, case)
        L.rl_set_wide_gemm(b"fp32")
        plan, _ = _plan(H, L, case, i, 0, 257)
        assert plan["rc"] == H.ERR_UNSUPPORTED and b"bf16 rows" in L.rl_last_error()
        # the reducers of every K-split plan over a sweep of few-tile shapes, with and without planes, in both tile settings
        seen = set()
        for tile in (b"auto", b"128"):
            for planes in (0, 1):
                G.restore_settings(L, mode0)
                L.rl_set_wide_gemm(b"bf16x3")
                L.rl_set_wgemm_tile(tile)
                for M in (1, 128, 500, 1000, 4000, 8000, 16000, 16300, 32000):
                    for N in (68, 128, 132, 192, 256, 260, 512, 1024):
                        for K in (256, 512, 1024, 2048):
                            d = H.GemmDesc()
                            d.A, d.lda, d.a_bstride, d.B, d.n, d.N, d.K = 0x1000000, K, M, 1, M, N, K
                            d.W, d.w_ks, d.w_ns, d.Y, d.ldy, d.y_bstride = 0x2000000, 1, K, 0x3000000, N, M
                            d.W_split = 0x4000000 if planes else None
                            d.kslab, d.kslab_floats = 0x5000000, 1 << 60
                            plan = H.gemm_plan(d)
                            assert plan["rc"] == 0
                            assert (plan["ksplit"] > 1) == (plan["reduce_cols"] != 0) == plan["kernel"].endswith("+splitk")
                            seen.add(plan["reduce_cols"])
        assert seen == {0, 16}
    finally:
        G.restore_settings(L, mode0)


# ---- the checker against the emulation and its mutants -------------------------------------------------------------------------------------
# (bf16 at K ~ 100: one dropped term is ~ 1 / K of the envelope on average, about the 2^-7 the bound allows, so it is caught on the
# elements where that term is larger than average - a few hundred outputs have them, a 2 x 48 product did not: the lattice's
# M = 1 edge cannot see this mutant in the bf16 mode at such K, its M >= 127 edges do)
SHAPES = [(129, 10, 13), (127, 64, 64), (385, 40, 132), (129, 128, 72), (65, 96, 48)]
MUTANTS = ["drop_k_tail", "last_row_from_previous", "swap_columns", "bias_twice", "accumulate_ignored", "lo_hi_missing",
           "operand_to_bf16", "leaky_as_relu"]


def _emulated(M, K, N, arith, mutant=None):
    """(Y, ref, env) of Y = act(A.scale + shift).W + bias + old Y: the fp32 emulation (or a mutant of it), the fp64 reference and
    its envelope.  A leaky lazy operand, a bias and an accumulating launch, so that every mutant has something to get wrong."""
    gen = torch.Generator().manual_seed(M * 1000 + K + N)
    A = torch.randn(M, K, generator=gen)
    scale, shift = torch.rand(K, generator=gen) + 0.5, torch.randn(K, generator=gen) * 0.3
    W = torch.randn(K, N, generator=gen) / K ** 0.5
    bias, old = torch.randn(N, generator=gen), torch.randn(M, N, generator=gen)
    z = A * scale + shift
    X32 = torch.relu(z) if mutant == "leaky_as_relu" else torch.where(z > 0, z, z * G.SLOPE)
    zd = A.double() * scale.double() + shift.double()
    X = torch.where(zd > 0, zd, zd * G.SLOPE)
    Xabs = (A.double() * scale.double()).abs() + shift.double().abs()
    ref = X @ W.double() + bias.double() + old.double()
    env = Xabs @ W.double().abs() + bias.double().abs() + old.double().abs()
    Xe, We = X32, W
    if mutant == "drop_k_tail":
        Xe = X32.clone()
        Xe[:, K - 1] = 0
    if mutant == "operand_to_bf16":
        Xe = X32.to(torch.bfloat16).to(torch.float32)
    Y = G.emulate_product(Xe, We, arith, drop_lo_hi=mutant == "lo_hi_missing")
    if mutant == "last_row_from_previous":
        Y[M - 1] = Y[M - 2]
    Y = Y + bias
    if mutant == "bias_twice":
        Y = Y + bias
    if mutant != "accumulate_ignored":
        Y = Y + old
    if mutant == "swap_columns":
        Y[:, [0, 1]] = Y[:, [1, 0]]
    return Y, ref, env


# (a_lo.w_hi exists in bf16x3 alone, and an operand rounded to bf16 is a mutant of the fp32 arithmetic alone)
PAIRS = [(a, m) for a in ("fp32", "bf16x3", "bf16") for m in MUTANTS
         if not ((m == "lo_hi_missing" and a != "bf16x3") or (m == "operand_to_bf16" and a != "fp32"))]


@pytest.mark.parametrize("arith", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_faithful_emulation_passes_with_the_stated_margin(M, K, N, arith):
    Y, ref, env = _emulated(M, K, N, arith)
    ratio = G.check(Y, ref, env, G.coefficient(arith, K), f"{arith} {M}x{K}x{N}")
    print(f"[lattice emulation] {arith} {M}x{K}x{N}: error / bound {ratio:.3f}")
    # (the margins the bound was accepted with: a correct product is well inside it, so a kernel near 1 is a finding)
    assert ratio <= {"fp32": 0.2, "bf16x3": 0.45, "bf16": 0.6}[arith]


@pytest.mark.parametrize("arith,mutant", PAIRS)
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_checker_rejects_the_mutant(M, K, N, arith, mutant):
    assert K <= 128
    Y, ref, env = _emulated(M, K, N, arith, mutant)
    with pytest.raises(AssertionError, match="x its bound"):
        G.check(Y, ref, env, G.coefficient(arith, K), mutant)


def test_the_bound_loses_power_as_k_grows():
    """Measured, not asserted against a kernel: the same arithmetic mutant (operand rounded to bf16 in the fp32 mode) sits further
    outside the bound at K = 64 than at K = 1024 - the bound grows as K, the mutant's error as sqrt(K)."""
    ratios = {}
    for K in (64, 1024):
        Y, ref, env = _emulated(129, K, 16, "fp32", "operand_to_bf16")
        err = (Y.double() - ref).abs()
        ratios[K] = float((err / (G.coefficient("fp32", K) * env)).max())
    print(f"[lattice emulation] operand rounded to bf16, error / fp32 bound: {ratios}")
    assert ratios[64] > 2 * ratios[1024]


def test_coefficients_are_the_derived_ones():
    assert G.coefficient("fp32", 10) == 18 * 2.0 ** -24
    assert G.coefficient("bf16x3", 64) == 3 * 2.0 ** -16 + 72 * 2.0 ** -24
    assert G.coefficient("bf16", 128) == 2.0 ** -7 + 2.0 ** -16 + 136 * 2.0 ** -24
