"""Host-side launch plans of the GEMM / weight-gradient families, pinned without a GPU.

The queries below (rl_gemm_stat_slots, rl_gemm_kslab_floats, rl_wgrad_slab_floats, rl_wgrad_nsplit, rl_gemm_streams,
rl_wgrad_batchable, rl_gemm_pair_supported) answer from the same planner rl_gemm / rl_wgrad launch from.  They are swept
over the network's shapes, the three arithmetic modes and the tile / staging / K-split settings, and compared with
tests/golden/gemm_plan.json.  Descriptors carry 16-byte-aligned dummy pointers: they are compared, never dereferenced,
and nothing is launched.

Regenerate the golden file (only when a plan is meant to change): python tests/test_gemm_plan_cpu.py
"""
import ctypes as C
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "gemm_plan.json")

MS = [1, 100, 2560, 10240, 40960, 327680]
WIDTHS = [3, 4, 10, 12, 16, 20, 32, 40, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1056]
MODES = ["fp32", "bf16x3", "bf16"]
TILES = ["auto", "128"]
STAGINGS = ["dma", "registers"]
KSPLITS = [0, 1]
QUERIES = ["rl_gemm_stat_slots", "rl_gemm_kslab_floats", "rl_wgrad_slab_floats", "rl_wgrad_nsplit",
           "rl_gemm_streams", "rl_wgrad_batchable", "rl_gemm_pair_supported"]

# dummy device addresses: 16-byte aligned, distinct, never dereferenced
_A, _W, _Y, _Y2, _WS, _WS2, _DY, _DW, _SLAB = (0x10000000 + 0x100000 * i for i in range(9))


def _gemm_desc(H, M, N, K, W_split, Y):
    d = H.GemmDesc()
    d.A, d.lda, d.a_bstride, d.a_mode = _A, K, M, 0
    d.B, d.n, d.N, d.K = 1, M, N, K
    d.W, d.w_ks, d.w_ns = _W, 1, K
    d.Y, d.ldy, d.y_bstride = Y, N, M
    d.W_split = W_split
    return d


def _wgrad_desc(H, M, N, K):
    d = H.WgradDesc()
    d.A, d.lda, d.a_bstride, d.a_mode = _A, K, M, 0
    d.B, d.n, d.N, d.K = 1, M, N, K
    d.dY, d.lddy, d.dy_bstride = _DY, N, M
    d.dW, d.w_ks, d.w_ns = _DW, 1, K
    d.slab, d.slab_floats = _SLAB, 1 << 62
    d.defer_reduce = 1
    return d


def _sweep(H, L):
    """{query: {setting: [value for M, K, N]}} under every setting; restores the defaults (and the mode) afterwards."""
    out = {q: {} for q in QUERIES}
    mode0 = L.rl_get_wide_gemm()
    try:
        for mode, tile, staging, ks in itertools.product(MODES, TILES, STAGINGS, KSPLITS):
            assert L.rl_set_wide_gemm(mode.encode()) == 0
            assert L.rl_set_wgemm_tile(tile.encode()) == 0
            assert L.rl_set_wgemm_staging(staging.encode()) == 0
            assert L.rl_set_gemm_ksplit(ks) == 0
            key = f"{mode}/{tile}/{staging}/{ks}"
            vals = {q: [] for q in QUERIES}
            for M, K, N in itertools.product(MS, WIDTHS, WIDTHS):
                vals["rl_gemm_stat_slots"].append(int(L.rl_gemm_stat_slots(M, N, K)))
                vals["rl_gemm_kslab_floats"].append(int(L.rl_gemm_kslab_floats(M, N, K)))
                vals["rl_wgrad_slab_floats"].append(int(L.rl_wgrad_slab_floats(M, N, K)))
                vals["rl_wgrad_nsplit"].append(int(L.rl_wgrad_nsplit(M, N, K)))
                a = _gemm_desc(H, M, N, K, _WS, _Y)
                vals["rl_gemm_streams"].append(int(L.rl_gemm_streams(C.byref(a))))
                vals["rl_wgrad_batchable"].append(int(L.rl_wgrad_batchable(C.byref(_wgrad_desc(H, M, N, K)))))
                b = _gemm_desc(H, M, N, K, _WS2, _Y2)
                vals["rl_gemm_pair_supported"].append(int(L.rl_gemm_pair_supported(C.byref(a), C.byref(b))))
            for q in QUERIES:
                out[q][key] = vals[q]
    finally:
        L.rl_set_wide_gemm(mode0)
        L.rl_set_wgemm_tile(b"auto")
        L.rl_set_wgemm_staging(b"dma")
        L.rl_set_gemm_ksplit(1)
    return out


def _pack(sweep):
    """Identical value lists are stored once: {"tables": [...], "queries": {query: {setting: table index}}}."""
    tables, index, queries = [], {}, {}
    for q, per in sweep.items():
        queries[q] = {}
        for key, vals in per.items():
            t = tuple(vals)
            if t not in index:
                index[t] = len(tables)
                tables.append(vals)
            queries[q][key] = index[t]
    return {"axes": {"M": MS, "K": WIDTHS, "N": WIDTHS, "modes": MODES, "tiles": TILES, "stagings": STAGINGS,
                     "ksplits": KSPLITS, "order": "M, K, N (N fastest)"},
            "tables": tables, "queries": queries}


def test_launch_plans_match_golden():
    from randlanet import _hip as H
    L = H.lib()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["axes"]["M"] == MS and golden["axes"]["K"] == WIDTHS and golden["axes"]["modes"] == MODES
    mode0 = L.rl_get_wide_gemm()
    got = _sweep(H, L)
    assert L.rl_get_wide_gemm() == mode0
    shapes = list(itertools.product(MS, WIDTHS, WIDTHS))
    for q in QUERIES:
        assert sorted(got[q]) == sorted(golden["queries"][q]), q
        for key, vals in got[q].items():
            want = golden["tables"][golden["queries"][q][key]]
            bad = [(shapes[i], v, w) for i, (v, w) in enumerate(zip(vals, want)) if v != w]
            assert not bad, f"{q} under {key}: (M, K, N), got, golden: {bad[:5]} ({len(bad)} differ)"


if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.join(REPO, "3d_recognizer_amd")]
    from randlanet import _hip as H
    packed = _pack(_sweep(H, H.lib()))
    with open(GOLDEN, "w") as f:
        json.dump(packed, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(packed['tables'])} distinct tables")
