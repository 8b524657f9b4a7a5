"""The demo's /frames route and the "frame" option of /click_pixel against a stand-in predictor that answers from the numpy reference
(tests/frames_reference.py): argument checking, the fused cloud, and a click on a photograph."""
import base64
import http.client
import json
import threading

import numpy as np
import torch

import frames_reference as R
import view_reference as V


class FakeFramer:
    """set_pointcloud / predict_masks as tests/test_demo_server_cpu.py's stand-in; set_frames / click_pixels answer from the numpy references."""

    def __init__(self):
        self.calls, self.frame_calls = [], []

    def set_pointcloud(self, xyz, rgb):
        self.xyz, self.rgb = xyz, rgb

    def predict_masks(self, pts, labels, prompt_mask, multimask):
        self.calls.append((pts.clone(), labels.clone()))
        logit = 0.5 - (self.xyz[0] - pts[0][-1]).norm(dim=-1)
        return logit[None, None], torch.tensor([[0.9]]), logit[None, None]

    def set_frames(self, depth, rgb, cameras, far, edge=0.05, depth_scale=None, max_points=None):
        from point_sam_amd.views import Camera, FrameSet, check_frame_cameras
        check_frame_cameras(cameras, "set_frames")
        self.frame_calls.append(dict(depth=depth, rgb=rgb, far=far, edge=edge, depth_scale=depth_scale, max_points=max_points))
        if R.unproject(depth, rgb, cameras, far, edge, depth_scale)[3] == 0:
            raise ValueError("frames_unproject: no pixel")
        out = R.frames(depth, rgb, cameras, far, edge, depth_scale)
        ncams = [Camera(n.pose_words.reshape(3, 4), n.fx, n.fy, n.cx, n.cy, n.width, n.height, n.near) for n in out["cams"]]
        return FrameSet(torch.from_numpy(out["keys"].view(np.int64)), ncams, torch.from_numpy(out["index"]), torch.from_numpy(out["xyz"]),
                        torch.from_numpy(out["rgb"]), out["center"], out["scale"])

    def click_pixels(self, view, pixels, labels, window=2):
        idx = V.pick(view.keys.numpy().view(np.uint64), pixels, window)
        if (idx < 0).any():
            raise ValueError(f"click_pixels: the click at pixel ({pixels[0][0]}, {pixels[0][1]}) hits no point within {window} pixels")
        return self.xyz[0][torch.from_numpy(idx).long()][None], torch.as_tensor(labels)[None]


def _req(port, method, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=20)
    c.request(method, path, None if body is None else json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def test_frames_route_and_clicks_on_a_photograph(tmp_path):
    from point_sam_amd.demo_server import DemoSession, serve
    depth, rgb, cams, far = R.room_case()
    mm, step = R.room_case_u16()
    specs = [{"pose": c.pose_words.reshape(3, 4).tolist(), "fx": c.fx, "fy": c.fy, "cx": c.cx, "cy": c.cy, "width": c.width, "height": c.height, "near": c.near}
             for c in cams]
    body = {"depth": _b64(depth), "rgb": _b64(rgb), "cameras": specs, "far": far}
    pred = FakeFramer()
    sess = DemoSession(pred, models_dir=str(tmp_path), output_dir=str(tmp_path / "results"), device="cpu")
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        port = srv.server_address[1]
        st, out = _req(port, "POST", "/click_pixel", {"pixel": [60, 45], "label": 1, "frame": 0})
        assert st == 400 and "point cloud" in out["error"]
        skew = dict(specs[1], pose=V.ROTATED.tolist())
        bad_bodies = [{}, {k: v for k, v in body.items() if k != "far"}, dict(body, extra=1), dict(body, cameras=[]), dict(body, cameras=specs[0]),
                      dict(body, cameras=[specs[0], 3]), dict(body, cameras=[specs[0], dict(specs[1], width=64)]), dict(body, cameras=[specs[0], dict(specs[1], fx=-1)]),
                      dict(body, cameras=specs[:1]), dict(body, cameras=[specs[0], skew]), dict(body, far=0), dict(body, far="10"), dict(body, far=True),
                      dict(body, edge=0), dict(body, edge=-0.05), dict(body, edge="x"), dict(body, depth_scale=0.001), dict(body, depth_scale=0, depth=_b64(mm)),
                      dict(body, depth=_b64(mm)), dict(body, depth=3), dict(body, depth="not base64!"), dict(body, rgb=_b64(rgb[:1])), dict(body, rgb=None),
                      dict(body, depth=_b64(np.zeros_like(depth)))]
        for bad in bad_bodies:
            st, out = _req(port, "POST", "/frames", bad)
            assert st == 400 and "error" in out, (st, {k: (v if k != "depth" and k != "rgb" else "...") for k, v in bad.items()})
        assert sess.pc_xyz is None and sess.frames is None
        assert "frame 1" in _req(port, "POST", "/frames", dict(body, cameras=[specs[0], skew]))[1]["error"]

        st, out = _req(port, "POST", "/frames", body)
        assert st == 200 and (out["frames"], out["width"], out["height"], out["num_points"]) == (2, 128, 96, R.ROOM_KEPT_EDGE)      # edge defaults to 0.05
        call = pred.frame_calls[-1]
        assert call["depth"].dtype == np.float32 and np.array_equal(call["depth"].view(np.uint32), depth.view(np.uint32)) and call["depth_scale"] is None
        assert call["rgb"].dtype == np.float32 and np.array_equal(call["rgb"], rgb.astype(np.float32) / np.float32(255))      # colours as /pointcloud/ has them
        assert call["edge"] == 0.05 and call["max_points"] == 2 * 96 * 128
        want = R.frames(depth, rgb.astype(np.float32) / np.float32(255), cams, far, 0.05)
        assert np.array_equal(np.array(out["xyz"], dtype=np.float32).reshape(-1, 3), want["xyz"]) and len(out["rgb"]) == 3 * R.ROOM_KEPT_EDGE
        assert np.allclose(out["center"], want["center"]) and np.isclose(out["scale"], want["scale"])
        assert sess.frames is not None and sess.view is None and tuple(sess.pc_xyz.shape) == (1, R.ROOM_KEPT_EDGE, 3)

        # a click on photograph 0 == a click on that pixel's own point through /segment
        st, out = _req(port, "POST", "/click_pixel", {"pixel": [60, 45], "label": 1})
        assert st == 400 and "before any /view" in out["error"]                  # without "frame" the route is what it was
        for bad in ({"pixel": [60, 45], "label": 1, "frame": 2}, {"pixel": [60, 45], "label": 1, "frame": -1}, {"pixel": [60, 45], "label": 1, "frame": 0.0},
                    {"pixel": [60, 45], "label": 1, "frame": True}, {"pixel": [60], "label": 1, "frame": 0}, {"pixel": [60, 45], "frame": 0},
                    {"pixel": [60, 45], "label": 1, "frame": 0, "extra": 1}):
            st, out = _req(port, "POST", "/click_pixel", bad)
            assert st == 400 and sess.prompts == [], bad
        st, out = _req(port, "POST", "/click_pixel", {"pixel": [60, 1], "label": 1, "frame": 0, "window": 0})
        assert st == 400 and "(60, 1)" in out["error"] and sess.prompts == []      # the zero rows show nothing
        own = int(want["index"][1, 45, 60])
        st, got = _req(port, "POST", "/click_pixel", {"pixel": [60, 45], "label": 1, "frame": 1})
        assert st == 200 and np.array_equal(np.array(sess.prompts[-1], dtype=np.float32), want["xyz"][own])
        assert _req(port, "POST", "/clear")[0] == 200
        st, direct = _req(port, "POST", "/segment", {"prompt_point": want["xyz"][own].tolist(), "prompt_label": 1})
        assert st == 200 and got == direct and torch.equal(pred.calls[-1][0], pred.calls[-2][0])

        # 16-bit depth with a scale, the edge filter off
        st, out = _req(port, "POST", "/frames", dict(body, depth=_b64(mm), depth_scale=step, edge=None))
        assert st == 200 and out["num_points"] == R.ROOM_KEPT
        call = pred.frame_calls[-1]
        assert call["depth"].dtype == np.uint16 and np.array_equal(call["depth"], mm) and call["depth_scale"] == step and call["edge"] is None
        # another cloud drops the frames
        sess.sampled_pointcloud({"points": {str(i): 0.1 * i for i in range(9)}, "colors": {str(i): 0.5 for i in range(9)}})
        st, out = _req(port, "POST", "/click_pixel", {"pixel": [60, 45], "label": 1, "frame": 0})
        assert st == 400 and "before any /frames" in out["error"]
    finally:
        srv.shutdown()
