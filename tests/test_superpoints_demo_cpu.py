"""The demo's /superpoints route and the --snap-superpoints option against a stand-in predictor that answers from the numpy reference
(tests/superpoint_reference.py): argument checking, the labels, and the proposal configuration /segment_all hands on."""
import http.client
import json
import threading

import numpy as np
import pytest
import torch

import region_reference as R
import superpoint_reference as SP


class FakeSegmenter:
    """set_pointcloud as tests/test_demo_server_cpu.py's stand-in; superpoints answers from the numpy reference; generate_masks records its config."""

    def __init__(self):
        self.sp_calls, self.proposal_cfgs = [], []

    def set_pointcloud(self, xyz, rgb):
        self.xyz = xyz

    def superpoints(self, cfg=None, cloud=0):
        from point_sam_amd.superpoints import Superpoints
        self.sp_calls.append(cfg)
        xyz = self.xyz[0].numpy()
        g = R.Graph(xyz, cfg.voxel_size)
        count, s, S = SP.scatter(xyz, g.inv, g.nbr)
        normal, curv, _, _ = SP.normals(count, s, S, cfg.min_points)
        vl, pl, size, num = SP.superpoints(g.inv, g.nbr, count, normal, curv, cfg.cos_angle, cfg.max_curvature, cfg.min_points, cfg.min_size,
                                           cfg.absorb_rounds)
        return Superpoints(torch.from_numpy(pl), torch.from_numpy(vl), torch.from_numpy(size), num, None)

    def generate_masks(self, cfg):
        from point_sam_amd.proposals import Proposals
        self.proposal_cfgs.append(cfg)
        n = self.xyz.shape[1]
        e = torch.empty(0)
        return [Proposals(n, torch.empty(0, (n + 63) // 64, dtype=torch.int64), e.long(), e.long(), e, e.int(), e, torch.full((n,), -1, dtype=torch.int32))]


def _req(port, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=20)
    c.request("POST", path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def _two_planes():
    g = np.arange(-16, 17) / 32.0
    a, b = np.meshgrid(g, g, indexing="ij")
    floor = np.stack([a.ravel(), b.ravel(), np.full(a.size, -0.5)], 1)
    wall = np.stack([np.full(a.size, -0.5), b.ravel(), a.ravel()], 1)
    return np.concatenate([floor, wall]).astype(np.float32)


def _upload(port, xyz):
    st, _ = _req(port, "/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten())},
                                               "colors": {str(i): 0.5 for i in range(xyz.size)}})
    assert st == 200


def test_superpoints_route_answers_with_labels_and_the_count():
    from point_sam_amd.demo_server import DemoSession, serve
    from point_sam_amd.superpoints import SuperpointConfig
    pred = FakeSegmenter()
    srv = serve(DemoSession(pred, device="cpu"), "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        st, out = _req(port, "/superpoints", {})
        assert st == 400 and "before a point cloud" in out["error"]
        xyz = _two_planes()
        _upload(port, xyz)
        st, out = _req(port, "/superpoints", {"config": {"voxel_size": 0.125}})
        assert st == 200 and out["num_superpoints"] == 2 and len(out["labels"]) == len(xyz)
        assert pred.sp_calls == [SuperpointConfig(voxel_size=0.125)]
        lab = np.array(out["labels"])
        assert set(lab.tolist()) == {0, 1} and lab[0] != lab[-1], "the floor's far corner and the wall's far corner lie in different superpoints"
        st, out = _req(port, "/superpoints", {"config": {"voxel_size": 0.125, "angle_deg": 91.0, "max_curvature": 1.0}})
        assert st == 200 and out["num_superpoints"] == 1 and set(out["labels"]) == {0}
        for bad in ({"config": {"nonsense": 1}}, {"config": {"min_size": -1}}, {"config": 3}, {"other": 1}, [1, 2]):
            st, out = _req(port, "/superpoints", bad)
            assert st == 400, bad
        assert len(pred.sp_calls) == 2, "a refused request never reaches the predictor"
    finally:
        srv.shutdown()


@pytest.mark.parametrize("flag", [False, True])
def test_snap_superpoints_option_sets_the_proposals_snap(flag):
    from point_sam_amd.demo_server import DemoSession, build_parser, serve
    from point_sam_amd.superpoints import SuperpointConfig
    assert build_parser().parse_args([]).snap_superpoints is False and build_parser().parse_args(["--snap-superpoints"]).snap_superpoints is True
    pred = FakeSegmenter()
    srv = serve(DemoSession(pred, device="cpu", snap_superpoints=flag), "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        _upload(port, _two_planes()[:200])
        assert _req(port, "/segment_all", {"num_prompts": 4})[0] == 200
        assert _req(port, "/segment_all", {"num_prompts": 4, "snap": {"min_size": 9}})[0] == 200
        a, b = pred.proposal_cfgs
        assert a.snap == (SuperpointConfig() if flag else None), "off by default: /segment_all is as before"
        assert b.snap == SuperpointConfig(min_size=9), "a request's own snap wins either way"
    finally:
        srv.shutdown()
    with pytest.raises(ValueError):
        DemoSession(pred, device="cpu", snap_superpoints=1)
