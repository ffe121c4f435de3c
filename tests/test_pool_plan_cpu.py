"""Host side of the fused pooling / virtual-rpe family (pool.hip), pinned without a GPU.

Plans: the size queries (rl_pool_slab_floats, rl_pool_bwd_slots, rl_pool_bwd_grid, rl_pool_fwd_slots, rl_rpe_stats_slots,
rl_rpe_wgrad_slab_floats) and rl_pool_supported answer from the same planner the five entries launch from.  They are swept over
the channel counts, stored / virtual, both stages, the three arithmetic modes and point counts on both sides of every grid cap,
and compared with tests/golden/pool_plan.json.

Refusals: a table of descriptors for rl_pool_fwd, rl_pool_bwd, rl_rpe_stats, rl_rpe_bn_reduce and rl_rpe_wgrad, each valid
except for one fault; the golden file holds the return code of each.  The descriptors carry 16-byte-aligned dummy addresses
that are never dereferenced - every case must be refused before anything is launched - which is why that test does not run
where a GPU is present: a validation bug must not be able to become a launch.

Regenerate the golden file (only when a plan or a return code is meant to change): python tests/test_pool_plan_cpu.py
"""
import ctypes as C
import itertools
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "pool_plan.json")

DS = [16, 32, 64, 128]
# both sides of every cap: 256 x 32, 768 x 16, 1024 x 16, 1280 x 16 points
POINTS = [1, 15, 16, 17, 31, 32, 33, 257, 2048, 4095, 4096, 8192, 12288, 16384, 20480, 40960, 327680]
MODES = ["fp32", "bf16x3", "bf16"]
QUERIES = ["rl_pool_supported", "rl_pool_supported/k8", "rl_pool_slab_floats", "rl_pool_bwd_slots", "rl_pool_bwd_grid/virtual0",
           "rl_pool_bwd_grid/virtual1", "rl_pool_fwd_slots", "rl_rpe_stats_slots", "rl_rpe_wgrad_slab_floats/stage1",
           "rl_rpe_wgrad_slab_floats/stage2"]
ENTRIES = ["rl_pool_fwd", "rl_pool_bwd", "rl_rpe_stats", "rl_rpe_bn_reduce", "rl_rpe_wgrad"]
POOL, RPE = ENTRIES[:2], ENTRIES[2:]


def _sweep(L):
    """{query: {mode: [value for d, points]}}; the arithmetic mode is restored afterwards."""
    out = {q: {} for q in QUERIES}
    mode0 = L.rl_get_wide_gemm()
    try:
        for mode in MODES:
            assert L.rl_set_wide_gemm(mode.encode()) == 0
            vals = {q: [] for q in QUERIES}
            for d, P in itertools.product(DS, POINTS):
                vals["rl_pool_supported"].append(int(L.rl_pool_supported(d, 16)))
                vals["rl_pool_supported/k8"].append(int(L.rl_pool_supported(d, 8)))
                vals["rl_pool_slab_floats"].append(int(L.rl_pool_slab_floats(P, d)))
                vals["rl_pool_bwd_slots"].append(int(L.rl_pool_bwd_slots(P, d)))
                vals["rl_pool_bwd_grid/virtual0"].append(int(L.rl_pool_bwd_grid(P, d, 0)))
                vals["rl_pool_bwd_grid/virtual1"].append(int(L.rl_pool_bwd_grid(P, d, 1)))
                vals["rl_pool_fwd_slots"].append(int(L.rl_pool_fwd_slots(P, d)))
                vals["rl_rpe_stats_slots"].append(int(L.rl_rpe_stats_slots(P)))
                vals["rl_rpe_wgrad_slab_floats/stage1"].append(int(L.rl_rpe_wgrad_slab_floats(P, d, 1)))
                vals["rl_rpe_wgrad_slab_floats/stage2"].append(int(L.rl_rpe_wgrad_slab_floats(P, d, 2)))
            for q in QUERIES:
                out[q][mode] = vals[q]
    finally:
        L.rl_set_wide_gemm(mode0)
    return out


def _pack(sweep):
    """Identical value lists are stored once: {"tables": [...], "queries": {query: {mode: table index}}}."""
    tables, index, queries = [], {}, {}
    for q, per in sweep.items():
        queries[q] = {}
        for key, vals in per.items():
            t = tuple(vals)
            if t not in index:
                index[t] = len(tables)
                tables.append(vals)
            queries[q][key] = index[t]
    return {"axes": {"d": DS, "points": POINTS, "modes": MODES, "order": "d, points (points fastest)"},
            "tables": tables, "queries": queries}


def test_size_queries_match_golden():
    from randlanet import _hip as H
    L = H.lib()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["axes"]["d"] == DS and golden["axes"]["points"] == POINTS and golden["axes"]["modes"] == MODES
    mode0 = L.rl_get_wide_gemm()
    got = _sweep(L)
    assert L.rl_get_wide_gemm() == mode0
    shapes = list(itertools.product(DS, POINTS))
    assert sorted(golden["queries"]) == sorted(QUERIES)
    for q in QUERIES:
        assert sorted(got[q]) == sorted(golden["queries"][q]), q
        for key, vals in got[q].items():
            want = golden["tables"][golden["queries"][q][key]]
            bad = [(shapes[i], v, w) for i, (v, w) in enumerate(zip(vals, want)) if v != w]
            assert not bad, f"{q} under {key}: (d, points), got, golden: {bad[:5]} ({len(bad)} differ)"


# ---- refusals ------------------------------------------------------------------------------------------------------
# dummy device addresses: 16-byte aligned, distinct, never dereferenced
_POINTERS = ["U", "u_scale", "u_shift", "G", "g_scale", "g_shift", "idx", "W", "Pout", "dP", "GU", "DG", "dW", "slab", "X_out",
             "dS_out", "xyz", "nbr_d2", "W1", "b1", "scale1", "shift1", "W2", "b2", "scale2", "shift2", "mean1", "invstd1", "mean2",
             "invstd2", "bn_bwd_stats", "bn_fwd_stats2", "pivot_mean1", "pivot_mean2", "arg_G", "arg_stats", "arg_coef", "arg_slab",
             "arg_GU1"]
_ADDR = {name: 0x10000000 + 0x100000 * i for i, name in enumerate(_POINTERS)}
_BIG = 1 << 62


def _required(entry, stage):
    """The pointers entry needs at this stage (0: a stored U): each of them null is one case."""
    branch = ["idx", "xyz", "nbr_d2", "W1", "b1"] + (["W2", "b2", "scale1", "shift1"] if stage == 2 else [])
    if entry in POOL:
        own = ["G", "idx", "W"] + (["Pout"] if entry == "rl_pool_fwd" else ["dP", "GU", "DG", "slab"])
        if stage == 0:
            return own + ["U"]
        return own + branch[1:] + (["scale1", "shift1"] if stage == 1 else ["scale2", "shift2"])
    records = ["scale1", "shift1", "mean1", "invstd1"] + (["scale2", "shift2", "mean2", "invstd2"] if stage == 2 else [])
    if entry == "rl_rpe_stats":
        return ["arg_stats"] + branch
    own = ["arg_G", "arg_stats"] if entry == "rl_rpe_bn_reduce" else ["arg_G", "arg_coef", "arg_slab"]
    return own + branch + [r for r in records if r not in branch]


class _Case:
    """A valid call of `entry` at `stage` (0: stored U) and width d under `mode`; `edit` then plants the one fault."""

    def __init__(self, entry, stage, d=64, mode="bf16x3"):
        self.entry, self.stage, self.mode = entry, stage, mode
        self.null_desc = False
        self.f = dict(points=2048, n=1024, d=d, nbr_k=16, g_bstride=1024, u_source=stage, xyz_bstride=1024, xyz_width=3,
                      slab_floats=_BIG)
        for name in _required(entry, stage) + (["X_out", "dS_out"] if d == 128 else []):
            self.f[name] = _ADDR[name]
        if entry in RPE:
            self.f["g_bstride"] = 0
            self.f["arg_slab_floats"] = _BIG
            if stage == 2:
                self.f["arg_GU1"] = _ADDR["arg_GU1"]

    def call(self, H, L):
        assert L.rl_set_wide_gemm(self.mode.encode()) == 0
        desc = H.PoolDesc()
        for k, v in self.f.items():
            if not k.startswith("arg_"):
                setattr(desc, k, v)
        a = lambda k: self.f.get("arg_" + k)
        ref = None if self.null_desc else C.byref(desc)
        if self.entry in POOL:
            return getattr(L, self.entry)(ref, None)
        if self.entry == "rl_rpe_stats":
            return L.rl_rpe_stats(ref, a("stats"), None)
        if self.entry == "rl_rpe_bn_reduce":
            return L.rl_rpe_bn_reduce(ref, a("G"), a("stats"), None)
        return L.rl_rpe_wgrad(ref, a("G"), a("coef"), a("slab"), a("slab_floats"), a("GU1"), None)


def _cases(L):
    """{name: _Case}: every descriptor valid except for the fault its name states."""
    out = {}

    def add(name, entry, stage, d=64, mode="bf16x3", null_desc=False, **edit):
        c = _Case(entry, stage, d, mode)
        c.null_desc = null_desc
        c.f.update(edit)
        key = f"{entry}/stage{stage}/{name}"
        assert key not in out, key
        out[key] = c

    for entry in ENTRIES:
        stages = (0, 1, 2) if entry in POOL else (1, 2)
        add("null descriptor", entry, stages[0], null_desc=True)
        for stage in stages:
            for name in _required(entry, stage):
                add(f"null {name}", entry, stage, **{name: None})
            add("points 0", entry, stage, points=0)
            add("points negative", entry, stage, points=-1024)
            add("n 0", entry, stage, n=0)
            add("points % n != 0", entry, stage, points=2047)
            add("nbr_k 8", entry, stage, nbr_k=8)
            add("d 48", entry, stage, d=48)
            add("points * 16 >= 2^31", entry, stage, points=1 << 27, n=1 << 20, g_bstride=(1 << 20) * (entry in POOL),
                xyz_bstride=1 << 20)
            add("u_source -1", entry, stage, u_source=-1)
            add("u_source 3", entry, stage, u_source=3)
            if stage == 0:
                add("d 128 in fp32 mode", entry, 0, d=128, mode="fp32")
                continue
            add("d 128 with a virtual stage", entry, stage, d=128)
            add("d 128 with a virtual stage, fp32 mode", entry, stage, d=128, mode="fp32")
            add("xyz_bstride < n", entry, stage, xyz_bstride=1023)
            add("n >= 2^24", entry, stage, points=1 << 24, n=1 << 24, g_bstride=(1 << 24) * (entry in POOL), xyz_bstride=1 << 24)
            add("row tensors of 2 GB", entry, stage, points=1 << 20, n=1 << 20, g_bstride=(1 << 20) * (entry in POOL),
                xyz_bstride=1 << 20)
            add("coordinate table of 2 GB", entry, stage, xyz_bstride=1 << 26)
            add("feature table of 2 GB", entry, stage, g_bstride=1 << 24)
            add("xyz_width 4 misaligned", entry, stage, xyz_width=4, xyz=_ADDR["xyz"] + 4)
        if entry in RPE:
            add("u_source 0", entry, 1, u_source=0)
            continue
        for stage in stages:
            add("g_bstride < n", entry, stage, g_bstride=1023)
            add("G misaligned", entry, stage, G=_ADDR["G"] + 4)
            add("g_scale without g_shift", entry, stage, g_scale=_ADDR["g_scale"])
            add("g_shift without g_scale", entry, stage, g_shift=_ADDR["g_shift"])
        add("U misaligned", entry, 0, U=_ADDR["U"] + 8)
        add("u_scale without u_shift", entry, 0, u_scale=_ADDR["u_scale"])
        add("u_shift without u_scale", entry, 0, u_shift=_ADDR["u_shift"])
        add("xyz_width 5", entry, 1, xyz_width=5)
        add("xyz_width 5", entry, 2, xyz_width=5)

    add("bn_fwd_stats2 with stage 2", "rl_pool_fwd", 2, bn_fwd_stats2=_ADDR["bn_fwd_stats2"], W2=_ADDR["W2"], b2=_ADDR["b2"])
    add("bn_fwd_stats2 with a stored U", "rl_pool_fwd", 0, bn_fwd_stats2=_ADDR["bn_fwd_stats2"], W2=_ADDR["W2"], b2=_ADDR["b2"])
    add("bn_fwd_stats2 without W2", "rl_pool_fwd", 1, bn_fwd_stats2=_ADDR["bn_fwd_stats2"], b2=_ADDR["b2"])
    add("bn_fwd_stats2 without b2", "rl_pool_fwd", 1, bn_fwd_stats2=_ADDR["bn_fwd_stats2"], W2=_ADDR["W2"])
    saved = dict(mean1=_ADDR["mean1"], invstd1=_ADDR["invstd1"], mean2=_ADDR["mean2"], invstd2=_ADDR["invstd2"])
    add("bn_bwd_stats with a stored U", "rl_pool_bwd", 0, bn_bwd_stats=_ADDR["bn_bwd_stats"], **saved)
    for stage in (1, 2):
        for miss in (f"mean{stage}", f"invstd{stage}"):
            add(f"bn_bwd_stats without {miss}", "rl_pool_bwd", stage, bn_bwd_stats=_ADDR["bn_bwd_stats"], **dict(saved, **{miss: None}))
    for mode in ("fp32", "bf16"):
        for stage in (0, 1, 2):
            add(f"rows_bf16 in {mode} mode", "rl_pool_bwd", stage, mode=mode, rows_bf16=1)
        for entry in ("rl_rpe_bn_reduce", "rl_rpe_wgrad"):
            for stage in (1, 2):
                add(f"rows_bf16 in {mode} mode", entry, stage, mode=mode, rows_bf16=1)
    # one float less than the launch's slabs take (the grids come from the size queries, pinned above)
    for d, stage in itertools.product((16, 64), (0, 1, 2)):
        grid = L.rl_pool_bwd_grid(2048, d, int(stage > 0))
        add(f"slab too small, d {d}", "rl_pool_bwd", stage, d=d, slab_floats=grid * (d * d + d) - 1)
        add(f"slab too small with dW, d {d}", "rl_pool_bwd", stage, d=d, dW=_ADDR["dW"], slab_floats=grid * d * d - 1)
    for d, stage in itertools.product((16, 64), (1, 2)):
        add(f"slab too small, d {d}", "rl_rpe_wgrad", stage, d=d, arg_slab_floats=L.rl_rpe_wgrad_slab_floats(2048, d, stage) - 1)
    add("stage 2 without GU1", "rl_rpe_wgrad", 2, arg_GU1=None)
    for mode in ("bf16x3", "bf16"):
        add(f"d 128 without X_out, {mode}", "rl_pool_bwd", 0, d=128, mode=mode, X_out=None)
        add(f"d 128 without dS_out, {mode}", "rl_pool_bwd", 0, d=128, mode=mode, dS_out=None)
        add(f"d 128 with X_out misaligned, {mode}", "rl_pool_bwd", 0, d=128, mode=mode, X_out=_ADDR["X_out"] + 4)
        add(f"d 128 with dS_out misaligned, {mode}", "rl_pool_bwd", 0, d=128, mode=mode, dS_out=_ADDR["dS_out"] + 8)
    return out


# Refused only since the five entries share one validation (rl_rpe_stats / rl_rpe_bn_reduce / rl_rpe_wgrad used to read any
# xyz_width other than 4 as 3): found by reading the code, not recorded - the golden file holds return codes of the revision
# before, where these descriptors would have been launched.
ERR_ARGS = -1
UNIFIED_ONLY = {f"{entry}/stage{stage}/xyz_width 5": ERR_ARGS for entry in RPE for stage in (1, 2)}


def _unified_only_cases():
    out = {}
    for key in UNIFIED_ONLY:
        entry, stage, _ = key.split("/")
        out[key] = _Case(entry, int(stage[-1]))
        out[key].f["xyz_width"] = 5
    return out


def _refusals(H, L, cases):
    """{name: return code}; every message must name its entry.  The arithmetic mode is restored afterwards."""
    mode0 = L.rl_get_wide_gemm()
    out = {}
    try:
        for key, case in cases.items():
            rc = int(case.call(H, L))
            msg = L.rl_last_error().decode("utf-8", "replace")
            assert rc != 0, f"{key}: accepted (the descriptor holds dummy addresses: it must be refused)"
            assert msg.startswith(case.entry + ":"), f"{key}: message {msg!r} does not start with {case.entry}"
            out[key] = rc
    finally:
        L.rl_set_wide_gemm(mode0)
    return out


def test_refusals_match_golden():
    import torch
    if torch.cuda.is_available():
        pytest.skip("the descriptors hold dummy device addresses: where a GPU is present a validation bug would become a launch")
    from randlanet import _hip as H
    L = H.lib()
    with open(GOLDEN) as f:
        golden = json.load(f)["refusals"]
    cases = _cases(L)
    assert sorted(cases) == sorted(golden)
    assert not set(UNIFIED_ONLY) & set(golden)
    mode0 = L.rl_get_wide_gemm()
    got = _refusals(H, L, cases)
    got.update(_refusals(H, L, _unified_only_cases()))
    assert L.rl_get_wide_gemm() == mode0
    want = dict(golden, **UNIFIED_ONLY)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"return codes (got, expected): {bad}"


if __name__ == "__main__":
    sys.path[:0] = [REPO, os.path.join(REPO, "3d_recognizer_amd")]
    import torch
    assert not torch.cuda.is_available(), "record without a GPU: the refusal descriptors hold dummy addresses"
    from randlanet import _hip as H
    L = H.lib()
    packed = _pack(_sweep(L))
    packed["refusals"] = _refusals(H, L, _cases(L))      # asserts that every case is refused
    with open(GOLDEN, "w") as f:
        json.dump(packed, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(packed['tables'])} distinct tables, {len(packed['refusals'])} refusals")
