"""Global registration on the MI355X: csrc/fpfh.hip, csrc/match.hip and csrc/global.hip against their numpy twins
(utils/features.py, utils/registration.py) on the cases of tests/global_inputs.py, bit for bit over every field, NaN positions
included; the entries' refusals and launches; global_registration and Model.predict_views(global_init=...) on device tensors
against the same steps done by hand."""
import numpy as np
import pytest
import torch

import global_inputs as gi
import registration_inputs as ri

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions")
        got, want = ri.bits(np.nan_to_num(got)), ri.bits(np.nan_to_num(want))
    assert np.array_equal(got, want), (what, np.flatnonzero((got != want).reshape(-1))[:8])


# ------------------------------------------------------------------------------------------------------- (a) descriptor
DESCRIPTOR_GRID = tuple(dict.fromkeys(f"{M}-{k}" for k in (2, 16, 63) for M in (k + 1, 63, 64, 65, 1023, 1025, 3000) if M >= k + 1))


@pytest.mark.parametrize("name", DESCRIPTOR_GRID + gi.DESCRIPTOR_SPECIALS)
def test_descriptor_equals_the_twin(name):
    from randlanet.utils.features import fpfh
    pts, nrm, k = gi.descriptor_case(name)
    got = fpfh(pts, k=k, normals=nrm, normal_k=min(16, pts.shape[0]), device=_dev())
    want = gi.descriptor_twin(name)
    for f in want._fields:
        _same_bits(getattr(got, f), getattr(want, f), (name, f))


def test_descriptor_specials_are_what_they_claim():
    t = gi.descriptor_twin
    assert (t("collinear").spfh == 0).all() and (t("collinear").code == 0).all()            # every pair skipped: lv2 = 0
    assert (t("zero_normals").spfh[::7] == 0).all() and t("zero_normals").spfh[1].sum() > 0
    assert t("along_normal").spfh[:, :11].sum(axis=1).max() < 16                            # the pair straight above is skipped
    assert t("duplicates").spfh[:40, :11].sum(axis=1).max() <= 14                           # two of the 16 ranks are copies
    assert t("planar").spfh.sum() > 0 and t("3000-16").spfh[:, :11].sum(axis=1).min() == 16


def test_descriptor_in_query_chunks():
    """3000 points in chunks of 1024 queries: rl_fpfh_spfh and rl_fpfh_fpfh run with first = 0, 1024 and 2048."""
    from randlanet import _ops as ops
    pts, _, k = gi.descriptor_case("3000-16")
    want = gi.descriptor_twin("3000-16")
    with torch.cuda.device(_dev()):
        desc, code, spfh = ops.fpfh(torch.from_numpy(pts).to(_dev()), torch.from_numpy(want.normals).to(_dev()), k, chunk=1024)
    _same_bits(desc.cpu().numpy(), want.descriptor, "descriptor")
    _same_bits(code.cpu().numpy(), want.code, "code")
    _same_bits(spfh.cpu().numpy(), want.spfh, "spfh")


# --------------------------------------------------------------------------------------------------------- (b) matching
@pytest.mark.parametrize("Mt", (1, 63, 65, 1000, 4097))
@pytest.mark.parametrize("Ms", (1, 63, 64, 65, 257, 1025))
def test_matching_equals_the_twin(Ms, Mt):
    from randlanet.utils.features import match_features, match_features_host
    cs, ct = gi.codes(Ms, Mt)
    idx, dist = match_features(cs, ct, device=_dev())
    widx, wdist = match_features_host(cs, ct)
    _same_bits(idx, widx, "idx")
    _same_bits(dist, wdist, "dist")
    if Mt >= 3 and Ms >= 3:
        assert dist[Ms // 2] == 0 and idx[Ms // 2] == 0          # the tie between rows 0 and Mt // 2 goes to the lower
        assert dist[Ms - 1] == 0
    if Mt == 1:
        assert dist[0] == 33 * 255 * 255


# ----------------------------------------------------------------------------------------------------------- (c) RANSAC
def _ransac_device(T, C, special=None):
    from randlanet import _ops as ops
    from randlanet.utils import registration as R
    src, tgt, corr, tri, es, md = gi.ransac_case(T, C, special)
    chk = R.check_global_parameters(md, iterations=T, edge_similarity=es)
    dev = _dev()
    with torch.cuda.device(dev):
        c = torch.from_numpy(corr).to(dev)
        M, count, inlier, best, counts, hyp, sums, status = ops.global_ransac(
            torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), c, tri, float(chk.s2), float(chk.g2))
        inlier = np.zeros(C, bool) if inlier is None else inlier.cpu().numpy()
    return R.GlobalRegistrationResult(M, count, count / C, inlier, corr, best, counts, hyp, sums, status)


@pytest.mark.parametrize("C", (3, 63, 65, 1025, 5000))
@pytest.mark.parametrize("T", (1, 63, 64, 65, 127, 129, 1025))
def test_ransac_equals_the_twin(T, C):
    gi.assert_same_global(_ransac_device(T, C), gi.ransac_twin(T, C), (T, C))


@pytest.mark.parametrize("special,T,C", [("repeated", 129, 1025), ("collinear", 65, 65), ("rejected", 1025, 1025),
                                         (None, 65, 1023), (None, 65, 1024), (None, 129, 66561)])
def test_ransac_specials_equal_the_twin(special, T, C):
    want = gi.ransac_twin(T, C, special)
    gi.assert_same_global(_ransac_device(T, C, special), want, (special, T, C))
    if special == "repeated":
        assert np.isnan(want.hypotheses[::2]).all() and want.status == "refined"
    if special in ("collinear", "rejected"):
        assert np.isnan(want.hypotheses).all() and want.status == "not_found" and want.best == -1 and not want.inlier.any()
        assert np.array_equal(want.transformation, np.eye(4)) and (want.sums == 0).all()
    if special is None:
        assert want.status == "refined" and want.count > C // 2         # the sums at 1023, 1024, 1025 (above) and 66561 rows


# ------------------------------------------------------------------------------------------------------- (d) end to end
@pytest.mark.parametrize("name", tuple(gi.PLANTED))
def test_planted_cases_equal_the_twin(name):
    from randlanet.utils.registration import global_registration
    src, tgt, _ = gi.planted(name)
    gi.assert_same_global(global_registration(src, tgt, device=_dev(), **gi.planted_keywords(name)), gi.planted_twin(name), name)


def test_global_registration_on_device_tensors():
    from randlanet.utils.registration import global_registration
    src, tgt, _ = gi.planted("rot40-small")
    dev = _dev()
    got = global_registration(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), **gi.planted_keywords("rot40-small"))
    gi.assert_same_global(got, gi.planted_twin("rot40-small"), "device tensors")


# ------------------------------------------------------------------------------------------------------ (e) the entries
def test_entries_refuse_bad_arguments_and_count_their_launches():
    from randlanet import _hip as H
    from randlanet import _ops as ops
    lib = H.lib()
    dev = _dev()
    src, tgt, corr, tri, es, md = gi.ransac_case(129, 1025)
    C, Mt, T = 1025, tgt.shape[0], 129
    cs, ct = gi.codes(257, 1000)
    with torch.cuda.device(dev):
        s, t, c, tr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (src, tgt, corr, tri))
        a, b = torch.from_numpy(cs).to(dev), torch.from_numpy(ct).to(dev)
        hyp = torch.empty((T, 12), dtype=torch.float32, device=dev)
        head = torch.empty(T + 1, dtype=torch.int32, device=dev)
        inl = torch.empty(C, dtype=torch.uint8, device=dev)
        out = torch.empty(16, dtype=torch.float64, device=dev)
        ws = ops.global_workspace(dev, C, T)
        mws = ops._workspace("rl_match_workspace_bytes", dev, 257, 1000)
        idx = torch.empty(257, dtype=torch.int64, device=dev)
        dist = torch.empty(257, dtype=torch.int32, device=dev)
        st = H.stream_ptr()
        rt = ops._icp_rt(np.eye(4))
        p = lambda x: x.data_ptr()
        good_h = [p(s), C, p(t), Mt, p(c), p(tr), T, 0.81, p(hyp), p(head), p(ws), ws.numel(), st]
        good_c = [p(s), C, p(t), Mt, p(c), p(hyp), T, 4e-4, p(head[1:]), p(ws), ws.numel(), st]
        good_s = [p(s), C, p(t), Mt, p(c), rt, 4e-4, p(inl), p(out), p(ws), ws.numel(), st]
        good_m = [p(a), 257, p(b), 1000, p(idx), p(dist), p(mws), mws.numel(), st]
        before = lib.rl_launch_count()

        def refused(fn, good, changes):
            for pos, value in changes:
                args = list(good)
                args[pos] = value
                assert fn(*args) == H.ERR_ARGS, (fn.__name__, pos, value)

        refused(lib.rl_global_hypotheses, good_h, [(1, 2), (1, 2 ** 31 - 1), (3, 0), (6, 0), (6, 2 ** 20 + 1), (7, 1.5), (7, -0.1),
                                                   (0, None), (4, None), (5, None), (8, None), (9, None), (10, None), (11, 16),
                                                   (10, p(ws) + 8)])
        refused(lib.rl_global_count, good_c, [(1, 2), (3, 0), (6, 0), (6, 2 ** 20 + 1), (7, 0.0), (7, float("inf")), (7, float("nan")),
                                              (0, None), (5, None), (8, None), (9, None), (10, 16)])
        refused(lib.rl_global_sums, good_s, [(1, 2), (3, 0), (6, 0.0), (6, float("nan")), (0, None), (5, None), (7, None), (8, None),
                                             (9, None), (10, 16)])
        refused(lib.rl_match_u8, good_m, [(1, 0), (1, 2 ** 31 - 1), (3, 0), (0, None), (2, None), (4, None), (5, None), (6, None),
                                          (7, 16), (0, p(a) + 1), (6, p(mws) + 8)])
        assert lib.rl_global_workspace_bytes(2, 1) == 0 and lib.rl_global_workspace_bytes(3, 2 ** 20 + 1) == 0
        assert lib.rl_match_workspace_bytes(0, 1) == 0 and lib.rl_match_workspace_bytes(1, 2 ** 31 - 1) == 0
        xyz = torch.from_numpy(gi.descriptor_case("65-16")[0]).to(dev)
        nrm = torch.from_numpy(gi.descriptor_twin("65-16").normals).to(dev)
        kidx, kd2 = ops.knn_f32(xyz[None], xyz[None], 17)
        before = lib.rl_launch_count()
        spfh = torch.empty((65, 33), dtype=torch.uint8, device=dev)
        desc = torch.empty((65, 33), dtype=torch.float32, device=dev)
        code = torch.empty((65, 36), dtype=torch.uint8, device=dev)
        good_p = [p(xyz), p(nrm), 65, p(kidx), p(kd2), 0, 65, 16, p(spfh), st]
        good_f = [p(spfh), 65, p(kidx), p(kd2), 0, 65, 16, p(desc), p(code), st]
        refused(lib.rl_fpfh_spfh, good_p, [(7, 1), (7, 64), (2, 16), (5, -1), (5, 1), (6, 0), (0, None), (1, None), (3, None),
                                           (4, None), (8, None)])
        refused(lib.rl_fpfh_fpfh, good_f, [(6, 1), (6, 64), (1, 16), (4, 1), (5, 66), (0, None), (2, None), (3, None), (7, None),
                                           (8, None)])
        assert lib.rl_launch_count() == before                                  # nothing was launched by a refused call
        assert lib.rl_fpfh_spfh(*good_p) == 0 and lib.rl_launch_count() == before + 1
        assert lib.rl_fpfh_fpfh(*good_f) == 0 and lib.rl_launch_count() == before + 2
        assert lib.rl_match_u8(*good_m) == 0 and lib.rl_launch_count() == before + 5
        assert lib.rl_global_hypotheses(*good_h) == 0 and lib.rl_launch_count() == before + 7
        assert lib.rl_global_count(*good_c) == 0 and lib.rl_launch_count() == before + 10
        assert lib.rl_global_sums(*good_s) == 0 and lib.rl_launch_count() == before + 12
        torch.cuda.synchronize()
        want = gi.descriptor_twin("65-16")
        _same_bits(code.cpu().numpy(), want.code, "code by the entries")
        assert int(head[0]) == 0
        tr[5, 1] = C                                                            # an index outside [0, C): flagged, nothing read
        assert lib.rl_global_hypotheses(*good_h) == 0
        assert int(head[0]) == 1 and bool(torch.isnan(hyp[5]).all())


# ------------------------------------------------------------------------------------------------- (f) Model.predict_views
def _model(use_gpu):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=use_gpu)


@pytest.mark.parametrize("to", ("first", "previous"))
def test_predict_views_with_global_init_on_a_gpu_placed_model(to):
    from randlanet.utils import registration as R
    model = _model(True)
    assert model.device.type == "cuda"
    views, motions = gi.views()
    vps = np.array([ri.moved_back(gi.VIEWPOINT[None], M)[0] for M in motions])
    icp = R.IcpSettings(max_distance=0.05)
    settings = R.GlobalSettings(voxel=0.04, iterations=4096, viewpoints=tuple(map(tuple, vps)))
    want, poses = gi.views_by_hand(model, views, icp, settings, to, _dev(), vps)
    np.random.seed(5)
    got, found = model.predict_views(views, icp=icp, to=to, global_init=settings, return_global=True, **ri.KW)
    assert found[0] is None and all(np.array_equal(ri.bits(found[v].transformation), ri.bits(poses[v])) for v in (1, 2))
    for g, w in zip(got.confidences, want.confidences):
        assert np.array_equal(ri.bits(g), ri.bits(w))
    assert np.array_equal(ri.bits(got.transformations), ri.bits(want.transformations)) and got.status == want.status
    assert np.array_equal(ri.bits(got.xyz), ri.bits(want.xyz))
    for v in (1, 2):
        rot, tr = ri.pose_error(got.transformations[v], motions[v])
        assert rot < 1.0 and tr < 0.01, (v, rot, tr)                    # (the bound of test_global_registration_cpu.py)
    # the CPU-placed model finds the same poses with the same bits, every field of every global result included
    np.random.seed(5)
    cpu, cpu_found = _model(False).predict_views(views, icp=icp, to=to, global_init=settings, return_global=True, **ri.KW)
    assert np.array_equal(ri.bits(cpu.transformations), ri.bits(got.transformations)) and np.array_equal(ri.bits(cpu.xyz), ri.bits(got.xyz))
    for v in (1, 2):
        gi.assert_same_global(found[v], cpu_found[v], (to, v))


def test_nothing_of_it_runs_without_global_init(monkeypatch):
    """global_init=None: none of the new wrappers is entered, and the call launches what it launched before they existed -
    the same number of kernels as the steps done by hand with icp and predict_scene on the same device tensors."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    from randlanet.utils import registration as R

    def never(*a, **k):
        raise AssertionError("entered without global_init")

    for name in ("fpfh", "match_features", "global_ransac", "global_workspace"):
        monkeypatch.setattr(ops, name, never)
    monkeypatch.setattr(R, "global_between", never)
    model = _model(True)
    views = [torch.from_numpy(v).to(model.device) for v in ri.views3()]
    icp = R.IcpSettings(0.08, iterations=10)
    lib = H.lib()
    np.random.seed(5)
    model.predict_views(views, icp=icp, **ri.KW)                        # (warm: every workspace size has been seen)
    torch.cuda.synchronize()
    before, held = lib.rl_launch_count(), torch.cuda.memory_allocated()
    np.random.seed(5)
    got = model.predict_views(views, icp=icp, global_init=None, **ri.KW)
    mine = lib.rl_launch_count() - before
    del got
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held                        # nothing new is kept
    before = lib.rl_launch_count()
    moved = [views[0]]
    chk = R.check_parameters(0.08, iterations=10, who="predict_views")
    for v in (1, 2):
        moved.append(R.icp_device(views[v], moved[0], None, chk, model.device).transformed)
    np.random.seed(5)
    model.predict_scene(torch.cat(moved, dim=0), None, **ri.KW)
    assert mine == lib.rl_launch_count() - before
