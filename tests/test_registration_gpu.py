"""Rigid registration on the MI355X: csrc/icp.hip against the numpy twin (utils/registration.py) on every case of
tests/registration_inputs.py, bit for bit over every field, `history` included; the entries' refusals, launches and
workspace; and icp / Model.predict_views on device tensors against the same steps done by hand."""
import numpy as np
import pytest
import torch

import registration_inputs as ri

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ (a) kernels against twin
@pytest.mark.parametrize("name", ri.CASES)
def test_device_equals_the_twin(name):
    from randlanet.utils.registration import icp
    src, tgt, kw = ri.case(name)
    ri.assert_same(icp(src, tgt, device=_dev(), **kw), ri.twin(name), name)


def test_special_cases_are_what_they_claim():
    assert ri.twin("gated_out").count == 0 and ri.twin("one_pair").count == 1
    assert (ri.twin("duplicates").correspondence < 1000).all() and ri.twin("zero_normals").count == 1000
    for m in ri.METRICS:
        assert ri.twin(f"planted-{m}-0.1").status == "converged" and ri.twin(f"{m}-66561-3000").history.shape[0] >= 3


@pytest.mark.parametrize("metric", ri.METRICS)
def test_query_chunks_start_past_the_first_row(metric):
    """5000 source points in chunks of 2048 queries: rl_icp_transform, rl_knn_f32 and rl_icp_sums run with first = 0, 2048
    and 4096, and the result is that of one chunk."""
    from randlanet.utils import registration as R
    tgt = ri.corner(3000, 3)
    rs = np.random.RandomState(9)
    src = ri.moved_back(tgt[rs.randint(0, 3000, 5000)] + rs.normal(0, 0.002, (5000, 3)), ri.motion(2.0, 0.4 * ri.SHIFT)).astype(F32)
    tgt = tgt.astype(F32)
    kw = dict(max_distance=0.08, metric=metric, iterations=4)
    want = R.icp_host(src, tgt, **kw)
    chk = R.check_parameters(**kw)
    res = R.icp_device(src, tgt, None, chk, _dev(), chunk=2048)
    got = res._replace(correspondence=res.correspondence.cpu().numpy(), transformed=res.transformed.cpu().numpy())
    ri.assert_same(got, want, "chunk 2048")
    ri.assert_same(R.icp(src, tgt, device=_dev(), **kw), want, "one chunk")
    assert want.updates >= 2 and want.count == 5000


# ------------------------------------------------------------------------------------------------ (b) the entries
def test_entries_refuse_bad_arguments_and_count_their_launches():
    from randlanet import _hip as H
    from randlanet import _ops as ops
    from randlanet.utils import registration as R
    from randlanet.utils.normals import estimate_normals_host
    lib = H.lib()
    src, tgt, _ = ri.case("point_to_plane-1025-300")
    src = np.concatenate([src, src[:1000] + F32(0.001), src[:475] + F32(0.5)])          # 2500 rows: three chunks
    nrm_h = estimate_normals_host(tgt, 16).normals
    T = ri.motion(1.5, 0.5 * ri.SHIFT)
    gate2 = float(F32(0.05) * F32(0.05))
    Ms, Mt = src.shape[0], tgt.shape[0]
    with torch.cuda.device(_dev()):
        s, t, nrm = (torch.from_numpy(np.array(a)).to(_dev()) for a in (src, tgt, nrm_h))
        q = torch.zeros((Ms, 3), dtype=torch.float32, device=_dev())
        corr = torch.full((Ms,), -7, dtype=torch.int64, device=_dev())
        out = torch.zeros(30, dtype=torch.float64, device=_dev())
        need = lib.rl_icp_workspace_bytes(Ms)
        ws = torch.zeros(need + 256, dtype=torch.uint8, device=_dev())
        rt = ops._icp_rt(T)
        idx = torch.zeros((Ms, 1), dtype=torch.int64, device=_dev())
        d2 = torch.zeros((Ms, 1), dtype=torch.float32, device=_dev())
        torch.cuda.synchronize()
        before = lib.rl_launch_count()
        good_t = [s.data_ptr(), Ms, 0, Ms, rt, q.data_ptr(), None]
        for pos, value in ((0, None), (4, None), (5, None), (1, 0), (1, 2 ** 31 - 1), (2, -1), (2, 1), (3, 0), (3, Ms + 1)):
            args = list(good_t)
            args[pos] = value
            assert lib.rl_icp_transform(*args) == H.ERR_ARGS, (pos, value)
        good_s = [q.data_ptr(), nrm.data_ptr(), t.data_ptr(), Mt, idx.data_ptr(), d2.data_ptr(), Ms, 0, Ms, gate2, 0,
                  corr.data_ptr(), ws.data_ptr(), need, None]
        for pos, value in ((0, None), (1, None), (2, None), (4, None), (5, None), (11, None), (12, None), (3, 0),
                           (3, 2 ** 31 - 1), (6, 0), (6, 2 ** 31 - 1), (7, -1024), (7, 512), (7, 1024), (8, 0), (8, 1000),
                           (8, Ms + 1), (9, 0.0), (9, -1.0), (9, float("nan")), (9, float("inf")), (10, 2), (10, -1),
                           (12, ws.data_ptr() + 8), (13, need - 1), (13, 0)):
            args = list(good_s)
            args[pos] = value
            assert lib.rl_icp_sums(*args) == H.ERR_ARGS, (pos, value)
        good_f = [Ms, out.data_ptr(), ws.data_ptr(), need, None]
        for pos, value in ((0, 0), (0, 2 ** 31 - 1), (1, None), (2, None), (2, ws.data_ptr() + 8), (3, need - 1), (3, 0)):
            args = list(good_f)
            args[pos] = value
            assert lib.rl_icp_fold(*args) == H.ERR_ARGS, (pos, value)
        assert lib.rl_launch_count() == before
        assert lib.rl_icp_transform(*good_t) == 0 and lib.rl_launch_count() == before + 1
        assert lib.rl_last_kernel() == b"icp_transform"
        idx, d2 = ops.knn_f32(t[None], q[None], 1)
        idx, d2 = idx[0].contiguous(), d2[0].contiguous()
        good_s[4], good_s[5] = idx.data_ptr(), d2.data_ptr()
        before = lib.rl_launch_count()
        assert lib.rl_icp_sums(*good_s) == 0 and lib.rl_launch_count() == before + 1
        assert lib.rl_last_kernel() == b"icp_sums"
        assert lib.rl_icp_fold(*good_f) == 0 and lib.rl_launch_count() == before + 2
        assert lib.rl_last_kernel() == b"icp_fold"
        torch.cuda.synchronize()
        # what the three entries wrote, against the twin's pieces
        want_row, want_corr, want_q = R.evaluate_host(src, tgt, nrm_h, T, F32(gate2), 0)
        assert np.array_equal(ri.bits(q.cpu().numpy()), ri.bits(want_q))
        assert np.array_equal(corr.cpu().numpy(), want_corr) and 0 < want_row[0] < Ms
        assert np.array_equal(ri.bits(out.cpu().numpy()), ri.bits(want_row))
        # the same sums from two calls, the second one starting at chunk 1; the point metric without normals
        out.zero_()
        corr.fill_(-7)
        for first, Q in ((0, 1024), (1024, Ms - 1024)):
            args = list(good_s)
            args[4], args[5], args[7], args[8] = idx[first:].data_ptr(), d2[first:].data_ptr(), first, Q
            assert lib.rl_icp_sums(*args) == 0
        assert lib.rl_icp_fold(*good_f) == 0
        assert np.array_equal(ri.bits(out.cpu().numpy()), ri.bits(want_row)) and np.array_equal(corr.cpu().numpy(), want_corr)
        args = list(good_s)
        args[1], args[10] = None, 1
        assert lib.rl_icp_sums(*args) == 0 and lib.rl_icp_fold(*good_f) == 0
        assert np.array_equal(ri.bits(out.cpu().numpy()), ri.bits(R.evaluate_host(src, tgt, None, T, F32(gate2), 1)[0]))
        # rows first .. first+Q-1 of the transform only
        q.zero_()
        args = list(good_t)
        args[2], args[3] = 100, 50
        assert lib.rl_icp_transform(*args) == 0
        got = q.cpu().numpy()
        assert np.array_equal(ri.bits(got[100:150]), ri.bits(want_q[100:150])) and not got[:100].any() and not got[150:].any()


def test_an_evaluation_adds_the_stated_launches():
    """_ops.icp with iterations = 0 on one chunk: rl_icp_transform, rl_icp_sums and rl_icp_fold are one launch each; the
    rest belongs to rl_knn_f32."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    from randlanet.utils import registration as R
    lib = H.lib()
    src, tgt, _ = ri.case("point_to_point-1025-3000")
    with torch.cuda.device(_dev()):
        s, t = torch.from_numpy(np.array(src)).to(_dev()), torch.from_numpy(np.array(tgt)).to(_dev())
        q = ops.icp_transform(s, np.eye(4))
        before = lib.rl_launch_count()
        ops.knn_f32(t[None], q[None], 1)
        knn = lib.rl_launch_count() - before
        before = lib.rl_launch_count()
        ops.icp(s, t, None, R.check_parameters(0.05, metric="point_to_point", iterations=0))
        assert lib.rl_launch_count() - before == 3 + knn


def test_workspace_bytes():
    from randlanet import _hip
    lib = _hip.lib()
    for Ms in (-1, 0, 2 ** 31 - 1, 2 ** 40):
        assert lib.rl_icp_workspace_bytes(Ms) == 0, Ms
    last = 0
    for Ms in (1, 1024, 1025, 66561, 501221, 10 ** 6, 2 ** 31 - 2):
        n = lib.rl_icp_workspace_bytes(Ms)
        chunks = -(-Ms // 1024)
        assert n % 256 == 0 and n >= last and 236 * chunks <= n <= 236 * chunks + 512, Ms
        last = n


# ------------------------------------------------------------------------------------------------ (c) composition
def _frames():
    """Two depth frames of one bumpy slope, the second seen 1.5 pixels to the side and 3 mm closer."""
    v, u = np.meshgrid(np.arange(48), np.arange(64), indexing="ij")

    def z(uu):
        return 300.0 + 40.0 * np.sin(uu / 9.0) * np.cos(v / 7.0) + 0.5 * uu

    return z(u).astype(np.uint16), (z(u + 1.5) - 3.0).astype(np.uint16)


def test_icp_on_device_tensors_from_depth_points():
    from randlanet.utils.depth import DepthCamera, depth_points
    from randlanet.utils.registration import apply_transform, icp, icp_host
    cam = DepthCamera(64, 48, 60.0, 60.0, 32.0, 24.0, 0.001)
    a, b = (depth_points(f, cam, device=_dev()).xyz for f in _frames())
    assert torch.is_tensor(a) and a.is_cuda and a.shape == (3072, 3) and b.shape == (3072, 3)
    kw = dict(max_distance=0.02, iterations=8)
    got = icp(b, a, **kw)                                       # device=None: the tensors say where
    assert isinstance(got.transformed, np.ndarray)
    want = icp_host(b.cpu().numpy(), a.cpu().numpy(), **kw)
    ri.assert_same(got, want, "depth")
    assert want.updates >= 1 and want.fitness > 0.5
    moved = apply_transform(b, got.transformation)
    assert torch.is_tensor(moved) and np.array_equal(ri.bits(moved.cpu().numpy()), ri.bits(want.transformed))
    assert np.array_equal(ri.bits(apply_transform(b.cpu().numpy(), got.transformation, device=_dev())), ri.bits(want.transformed))
    with pytest.raises(ValueError, match="source"):
        icp(b.double(), a, **kw)
    bad = a.clone()
    bad[7, 2] = float("inf")
    with pytest.raises(ValueError, match="target"):
        icp(b, bad, **kw)


def _model(use_gpu):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=use_gpu)


@pytest.mark.parametrize("to", ("first", "previous"))
def test_predict_views_on_a_gpu_placed_model(to):
    from randlanet.utils.registration import IcpSettings
    model = _model(True)
    assert model.device.type == "cuda"
    views = ri.views3()
    settings = IcpSettings(0.08, iterations=10)
    np.random.seed(5)
    got = model.predict_views(views, icp=settings, to=to, **ri.KW)
    want, T, xyz = ri.by_hand(model, views, settings, to, _dev())
    assert np.array_equal(ri.bits(got.transformations), ri.bits(T)) and np.array_equal(ri.bits(got.xyz), ri.bits(xyz))
    assert [c.shape for c in got.confidences] == [(4, 700), (4, 600), (4, 500)]
    assert np.array_equal(ri.bits(np.concatenate(got.confidences, axis=1)), ri.bits(want))
    # device tensors as views stay where they are and give the same result
    np.random.seed(5)
    dev = model.predict_views([torch.from_numpy(v).to(model.device) for v in views], icp=settings, to=to, **ri.KW)
    assert all(np.array_equal(ri.bits(a), ri.bits(b)) for a, b in zip(dev.confidences, got.confidences))
    assert np.array_equal(ri.bits(dev.transformations), ri.bits(T))
    # the CPU-placed model registers with the same bits
    np.random.seed(5)
    cpu = _model(False).predict_views(views, icp=settings, to=to, **ri.KW)
    assert np.array_equal(ri.bits(cpu.transformations), ri.bits(T)) and np.array_equal(ri.bits(cpu.xyz), ri.bits(xyz))
    assert cpu.status == got.status and np.array_equal(cpu.fitness, got.fitness) and np.array_equal(cpu.inlier_rmse, got.inlier_rmse)
