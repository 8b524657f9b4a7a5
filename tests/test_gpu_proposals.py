"""Automatic mask proposals on the GPU (csrc/masks.hip, point_sam_amd/proposals.py): every result is an integer or a copy, so every comparison is
equality -- against the plain numpy reference in tests/mask_reference.py and against the existing `decode`, never against the new code's other path."""
import http.client
import json
import threading

import numpy as np
import pytest
import torch

import mask_reference as R
from oracle import pointsam_oracle as O
from point_sam_amd.config import get_config
from point_sam_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops
    return ops


def _np_words(t):
    return t.cpu().numpy().view(np.uint64)


def _dev_words(masks):
    return torch.from_numpy(R.words(masks).view(np.int64)).cuda()


# ------------------------------------------------------------------------------------------------ 1. pack
@pytest.mark.parametrize("N", [64, 2048, 2048 + 37, 32768])
def test_pack_equals_numpy(ops, N):
    """Bits, tail bits and the three areas; exact-threshold values, -0.0, NaN and infinities; the source a cloud's slice of a [Z, 3, N] tensor, the
    destination a row offset of a larger buffer whose other rows stay untouched."""
    rng = np.random.default_rng(N)
    thr, off = f32(0.25), f32(0.5)
    Z, C, B = 6, 3, 2                                     # two clouds, chunk of 3 prompts each
    L = rng.normal(0.25, 1.0, (Z, C, N)).astype(f32)
    special = np.array([thr, thr + off, thr - off, np.nextafter(thr, f32(1)), np.nextafter(thr, f32(-1)), -0.0, 0.0, np.nan, np.inf, -np.inf,
                        np.nextafter(f32(thr + off), f32(9)), np.nextafter(f32(thr - off), f32(9))], dtype=f32)
    L.reshape(-1)[rng.choice(L.size, L.size // 8, replace=False)] = rng.choice(special, L.size // 8)
    L[0, 0, :] = np.nan; L[0, 1, :] = np.inf; L[0, 2, :] = thr; L[1, 0, -1] = np.inf; L[1, 1, 0] = np.inf
    dev = torch.from_numpy(L).cuda()
    W = ops.mask_words(N)
    K = 40
    for b, row in ((1, 9 * 3), (0, 0)):                   # cloud b's slice -> rows row .. row + 8
        src = dev[b * 3:(b + 1) * 3]
        assert src.data_ptr() != dev.data_ptr() or b == 0
        bufs = (torch.full((K, W), -1, dtype=torch.int64, device="cuda"),) + tuple(torch.full((K,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        out = ops.mask_pack(src, float(thr), float(off), out=bufs, row=row)
        assert all(o is t for o, t in zip(out, bufs))
        m, area, hi, lo = R.pack(L[b * 3:(b + 1) * 3].reshape(9, N), thr, off)
        want = R.words(m)
        got = _np_words(bufs[0])
        assert np.array_equal(got[row:row + 9], want)
        if N % 64:
            assert (got[row:row + 9, -1] >> np.uint64(N % 64)).max() == 0, "tail bits must be zero"
        for t, w in zip(bufs[1:], (area, hi, lo)):
            assert np.array_equal(t.cpu().numpy()[row:row + 9], w.astype(np.int32))
            rest = np.delete(t.cpu().numpy(), np.s_[row:row + 9])
            assert (rest == -7).all()
        assert (np.delete(bufs[0].cpu().numpy(), np.s_[row:row + 9], axis=0) == -1).all(), "rows outside the destination range were written"
    # the plain call: fresh buffers, [K, N] input, default threshold 0 / offset 1: -0.0 and 0.0 are both "not above 0"
    bits, area, hi, lo = ops.mask_pack(dev.view(Z * C, N))
    m, a0, h0, l0 = R.pack(L.reshape(Z * C, N), 0.0, 1.0)
    assert np.array_equal(_np_words(bits), R.words(m)) and np.array_equal(area.cpu().numpy(), a0) and np.array_equal(hi.cpu().numpy(), h0)
    assert np.array_equal(lo.cpu().numpy(), l0)
    assert area[0].item() == 0 and area[1].item() == N and np.array_equal(ops.mask_unpack(bits, N).cpu().numpy(), m)


# ------------------------------------------------------------------------------------------------ 2. intersections
@pytest.mark.parametrize("Ka,Kb,W", [(1, 1, 1), (5, 130, 7), (192, 192, 33), (65, 64, 70), (3072, 3072, 512)])
def test_intersections_equal_numpy(ops, Ka, Kb, W):
    rng = np.random.default_rng(Ka * 7 + Kb)
    N = W * 64 - (0 if W in (1, 512) else 29)
    big = Ka * Kb * N > 1 << 31
    a = rng.random((Ka, N)) < rng.uniform(0.02, 0.6, (Ka, 1))
    b = rng.random((Kb, N)) < rng.uniform(0.02, 0.6, (Kb, 1))
    a[0] = True; b[-1] = False
    da, db = _dev_words(a), _dev_words(b)
    got = ops.mask_intersections(da, db)
    assert got.dtype == torch.int32 and tuple(got.shape) == (Ka, Kb)
    assert np.array_equal(got.cpu().numpy(), R.intersections(a, b, exact_int=not big))
    # a against itself: the mirrored upper triangle
    sym = ops.mask_intersections(da).cpu().numpy()
    assert np.array_equal(sym, sym.T) and np.array_equal(np.diag(sym), a.sum(1))
    if not big:
        assert np.array_equal(sym, R.intersections(a, a))
    else:      # one fp32 matmul of this size is enough: the general path below is checked against it, the mirrored path against the general one
        assert np.array_equal(ops.mask_intersections(db, da).cpu().numpy(), got.cpu().numpy().T)
    assert np.array_equal(ops.mask_intersections(da, da.clone()).cpu().numpy(), sym)      # the general path on the same data


# ------------------------------------------------------------------------------------------------ 3. validity + nms + paint on blobs
def _blobs():
    rng = np.random.default_rng(0)
    N, K = 8192, 256
    p = rng.uniform(-1, 1, (N, 3)).astype(f32)
    c = p[rng.choice(N, K, replace=False)]
    r = rng.uniform(0.15, 0.6, K).astype(f32)
    L = ((r[:, None] - np.linalg.norm(p[None] - c[:, None], axis=-1)) * 8 + rng.normal(0, 0.1, (K, N))).astype(f32)
    S = rng.uniform(0, 1, K).astype(f32)
    return N, K, L, S


def _device_post(ops, L, S, N, thr, off, min_points, max_area_frac, pred_iou_thr, stab_thr, nms_thr):
    bits, area, hi, lo = ops.mask_pack(torch.from_numpy(L).cuda(), thr, off)
    score = torch.from_numpy(S).cuda()
    order = torch.sort(score, descending=True, stable=True).indices.to(torch.int32)
    valid = ops.mask_valid(area, hi, lo, score, N, min_points, max_area_frac, pred_iou_thr, stab_thr)
    inter = ops.mask_intersections(bits)
    keep = ops.mask_nms(order, valid, area, inter, nms_thr)
    labels = ops.mask_paint(bits, order, keep, N)
    return dict(bits=bits, area=area, valid=valid, order=order, inter=inter, keep=keep, labels=labels)


def _assert_post_equal(got, want, tag):
    assert np.array_equal(got["area"].cpu().numpy(), want["area"]), tag
    assert np.array_equal(got["valid"].cpu().numpy().astype(bool), want["valid"]), tag
    assert np.array_equal(got["inter"].cpu().numpy(), want["inter"]), tag
    nk, ns = int(want["keep"].sum()), int((want["valid"] & ~want["keep"]).sum())
    print(f"{tag}: valid {int(want['valid'].sum())}, reference keeps {nk}, suppresses {ns}; device keeps {int(got['keep'].sum())}")
    assert np.array_equal(got["keep"].cpu().numpy().astype(bool), want["keep"]), tag
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"]), tag
    return nk, ns


def test_nms_validity_paint_on_blobs(ops):
    """256 noisy balls on 8192 points (areas 7 .. 925): the numpy reference keeps 221 of 256 at IoU 0.5 and 137 at 0.3 with no filter, 55 and 39 of the
    64 that pass a score and stability cut at their medians.  keep and labels must equal the reference; the reference itself must keep at least 32 and
    suppress at least 7 in each setting (a condition on the inputs: an all-kept or all-dropped case cannot pass for equality)."""
    N, K, L, S = _blobs()
    _, area, hi, lo = R.pack(L, 0.0, 0.5)
    assert area.min() > 0 and area.max() < N
    s_med, st_med = f32(np.median(S)), f32(np.median(hi / lo))
    for pred_iou, stab, nms_thr in ((-np.inf, 0.0, 0.5), (-np.inf, 0.0, 0.3), (s_med, st_med, 0.5), (s_med, st_med, 0.3)):
        want = R.proposals(L, S, N, 0.0, 0.5, 1, 1.0001, pred_iou, stab, nms_thr)
        got = _device_post(ops, L, S, N, 0.0, 0.5, 1, 1.0001, float(pred_iou), float(stab), nms_thr)
        nk, ns = _assert_post_equal(got, want, f"blobs iou>={pred_iou} stab>={stab} nms {nms_thr}")
        assert nk >= 32 and ns >= 7
    # ties: equal scores keep the lower index first, and a mask duplicated outright (IoU exactly 1) loses to its earlier twin
    L2, S2 = L.copy(), S.copy()
    S2[10] = S2[200]; S2[50] = S2[51] = S2[52]; S2[255] = S2[0]
    L2[77] = L2[33]; S2[77] = S2[33]
    L2[5] = L2[140]; S2[5] = np.nextafter(S2[140], f32(-1))        # a twin with a slightly lower score
    L2[250] = L2[140]; S2[250] = S2[140]                           # and one with the same score: the higher index comes later and must go
    for nms_thr in (0.5, 1.0):      # at 1.0 nothing overlaps "more than completely": only the filter decides
        want = R.proposals(L2, S2, N, 0.0, 0.5, 1, 1.0001, -np.inf, 0.0, nms_thr)
        got = _device_post(ops, L2, S2, N, 0.0, 0.5, 1, 1.0001, float("-inf"), 0.0, nms_thr)
        assert np.array_equal(got["order"].cpu().numpy(), want["order"])
        _assert_post_equal(got, want, f"ties nms {nms_thr}")
        if nms_thr == 0.5:
            assert not want["keep"][77] and not want["keep"][5] and want["keep"][140] and not want["keep"][250]
            assert want["inter"][77, 33] == want["area"][33] == want["area"][77]
        else:
            assert want["keep"].all()
    # the area filter of the reference's instance masks: at least 25 points, under 90 % of the cloud; an invalid best candidate suppresses nothing
    L3 = L.copy(); L3[3] = 1.0; L3[4] = -1.0
    S3 = S.copy(); S3[3] = 2.0; S3[9] = np.nan
    want = R.proposals(L3, S3, N, 0.0, 0.5, 25, 0.9, 0.0, 0.0, 0.5)
    got = _device_post(ops, L3, S3, N, 0.0, 0.5, 25, 0.9, 0.0, 0.0, 0.5)
    assert not want["valid"][3] and not want["valid"][4] and not want["valid"][9] and want["keep"].sum() >= 32
    _assert_post_equal(got, want, "area filter")


# ------------------------------------------------------------------------------------------------ 4. end to end
def _reference_run(model, ops, st, num_prompts, chunk):
    """The existing decode with the same chunking as generate_proposals (same Z per call: the same bits), logits to the host."""
    B, N, _ = st.coords.shape
    _, prompts = ops.fps(st.coords, num_prompts)
    logits, scores = [[] for _ in range(B)], [[] for _ in range(B)]
    for m0 in range(0, num_prompts, chunk):
        c = min(chunk, num_prompts - m0)
        pts = prompts[:, m0:m0 + c].reshape(B * c, 1, 3)
        masks, iou = model.decode(st, pts, torch.ones(B * c, 1, dtype=torch.int64, device="cuda"), None, True)
        for b in range(B):
            logits[b].append(masks[b * c:(b + 1) * c].reshape(-1, N).cpu().numpy())
            scores[b].append(iou[b * c:(b + 1) * c].reshape(-1).cpu().numpy())
    model.check_coordinate_range()
    return [np.concatenate(x) for x in logits], [np.concatenate(x) for x in scores]


@pytest.mark.parametrize("B,num_prompts,chunk", [(1, 64, 16), (2, 64, 16), (1, 40, 16)])
def test_generate_proposals_equals_decode_plus_numpy(ops, B, num_prompts, chunk):
    """Tiny model, random weights (seed 3), 2048 points.  Random weights give degenerate masks at threshold 0 (most candidates cover everything or
    nothing), so the threshold is the fp32 median of the reference logits; no area filter.  The reference must keep at least 8 and suppress at
    least 8 before anything is compared.  Second run: the score cut at the median score.  (1, 40, 16): a short last chunk."""
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.proposals import ProposalConfig, generate_proposals
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    xyz, rgb, _, _ = O.synthetic_batch(B, 2048, seed=8)
    st = model.encode(xyz.cuda(), rgb.cuda())
    N = 2048
    logits, scores = _reference_run(model, ops, st, num_prompts, chunk)
    thr = float(f32(np.median(np.concatenate(logits))))
    for pred_iou in (float("-inf"), float(f32(np.median(np.concatenate(scores))))):
        pc = ProposalConfig(num_prompts=num_prompts, prompt_chunk=chunk, mask_threshold=thr, pred_iou_thresh=pred_iou, stability_thresh=0.0,
                            stability_offset=1.0, nms_thresh=0.7, min_points=1, max_area_frac=1.0001)
        got = generate_proposals(model, st, pc)
        assert len(got) == B
        for b in range(B):
            want = R.proposals(logits[b], scores[b], N, thr, 1.0, 1, 1.0001, pred_iou, 0.0, 0.7)
            nk, ns = int(want["keep"].sum()), int((want["valid"] & ~want["keep"]).sum())
            print(f"B={B} P={num_prompts} cloud {b} thr {thr:.4f} score cut {pred_iou}: non-empty {int((want['area'] > 0).sum())}, valid "
                  f"{int(want['valid'].sum())}, reference keeps {nk}, suppresses {ns}; device keeps {len(got[b])}")
            if pred_iou == float("-inf") and num_prompts == 64:
                assert nk >= 8 and ns >= 8, (nk, ns)
            p, cand = got[b], want["candidate"]
            assert np.array_equal(p.candidate.cpu().numpy(), cand)
            assert np.array_equal(p.prompt_index.cpu().numpy(), cand // 3)
            assert np.array_equal(p.score.cpu().numpy(), scores[b][cand])
            assert np.array_equal(p.area.cpu().numpy(), want["area"][cand])
            assert np.array_equal(p.labels.cpu().numpy(), want["labels"])
            assert np.array_equal(p.masks().cpu().numpy(), want["masks"][cand])
            assert np.array_equal(_np_words(p.bits), R.words(want["masks"][cand]))
            assert np.array_equal(p.stability.cpu().numpy(), want["area_hi"][cand].astype(f32) / want["area_lo"][cand].astype(f32))
            assert p.labels.dtype == torch.int32 and p.candidate.dtype == torch.int64 and p.n_points == N


def test_fps_prompts_are_a_prefix_of_the_cached_centers(ops):
    """FPS from index 0 is prefix-consistent: the first num_prompts group centres of the encoder state are the prompt grid."""
    from point_sam_amd.model import PointCloudSAM
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda")
    xyz, rgb, _, _ = O.synthetic_batch(2, 2048, seed=8)
    st = model.encode(xyz.cuda(), rgb.cuda())
    P = min(48, st.centers.shape[1])
    idx, pts = ops.fps(st.coords, P)
    assert torch.equal(idx, st.fps_idx[:, :P]) and torch.equal(pts, st.centers[:, :P])


# ------------------------------------------------------------------------------------------------ 5. no hidden sync: capturable
def test_everything_before_the_compaction_is_capturable(ops):
    """propose_on_device (FPS, the chunked decodes, pack, sort, validity, intersections, NMS, paint) inside a graph capture on a side stream: a host
    synchronisation anywhere in it would fail the capture.  The replay equals the eager result."""
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.proposals import ProposalConfig, compact, generate_proposals, propose_on_device
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    xyz, rgb, _, _ = O.synthetic_batch(2, 2048, seed=8)
    st = model.encode(xyz.cuda(), rgb.cuda())
    logits, _ = _reference_run(model, ops, st, 32, 16)
    pc = ProposalConfig(num_prompts=32, prompt_chunk=16, mask_threshold=float(f32(np.median(np.concatenate(logits)))), pred_iou_thresh=float("-inf"),
                        stability_thresh=0.0, min_points=1, max_area_frac=1.0001)
    want = generate_proposals(model, st, pc)
    cap = torch.cuda.Stream()
    block = ops.new_counters(st.coords.device)
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap), ops.use_counters(block):
        propose_on_device(model, st, pc)                  # warm-up on the capture stream
    cap.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap), ops.use_counters(block):
        dev = propose_on_device(model, st, pc)
    torch.cuda.synchronize()
    for _ in range(2):
        for d in dev:
            d.keep.zero_(); d.labels.fill_(-5); d.bits.zero_()
        g.replay()
        torch.cuda.synchronize()
        for d, w in zip(dev, want):
            p = compact(d)
            assert len(p) == len(w) and len(p) >= 1
            for name in ("bits", "candidate", "prompt_index", "score", "area", "stability", "labels"):
                assert torch.equal(getattr(p, name), getattr(w, name)), name
    model.check_coordinate_range()


# ------------------------------------------------------------------------------------------------ 6. predictor, recall, demo
def test_predictor_generate_masks(ops):
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.proposals import ProposalConfig, generate_proposals
    cfg = get_config("tiny")
    model = PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3")
    pred = PointSAMPredictor(model)
    with pytest.raises(RuntimeError, match="set_pointcloud"):
        pred.generate_masks()
    xyz, rgb, _, _ = (t.cuda() for t in O.synthetic_batch(1, 2048, seed=8))
    pred.set_pointcloud(xyz, rgb)
    pc = ProposalConfig(num_prompts=32, prompt_chunk=32, mask_threshold=1.5, pred_iou_thresh=float("-inf"), stability_thresh=0.0, min_points=1,
                        max_area_frac=1.0001)
    got = pred.generate_masks(pc)
    want = generate_proposals(model, model.encode(xyz, rgb), pc)
    assert len(got) == 1 and torch.equal(got[0].bits, want[0].bits) and torch.equal(got[0].labels, want[0].labels)
    k = len(got[0])
    assert int(got[0].labels.max()) < max(k, 1) and int(got[0].labels.min()) >= -1
    assert len(pred.generate_masks()) == 1                # the defaults run
    with pytest.raises(ValueError):                       # prompts outside [-1, 1] are still refused
        bad = PointSAMPredictor(model)
        bad.set_pointcloud(xyz * 3, rgb)
        bad.generate_masks(pc)


def test_proposal_recall_equals_numpy_iou_table(ops):
    from point_sam_amd.evaluation import proposal_recall
    from point_sam_amd.proposals import Proposals
    N, K, L, S = _blobs()
    m, area, _, _ = R.pack(L, 0.0, 0.5)
    sel = np.arange(0, K, 4)                              # 64 blobs as the "proposals"
    z = torch.zeros(len(sel), device="cuda")
    prop = Proposals(N, _dev_words(m[sel]), torch.from_numpy(sel).cuda(), torch.from_numpy(sel // 3).cuda(), z, torch.from_numpy(area[sel].astype(np.int32)).cuda(),
                     z + 1, torch.zeros(N, dtype=torch.int32, device="cuda"))
    thresholds = (0.25, 0.5, 0.75, 1.0)
    same = proposal_recall(prop, torch.from_numpy(m[sel]).cuda(), thresholds)
    assert (same["best_iou"] == 1.0).all() and (same["recall"] == 1.0).all()
    gt = np.roll(m, 1, axis=0)[::2]                       # a shifted set: some blobs are proposals, most are only overlapped by one
    out = proposal_recall(prop, torch.from_numpy(gt), thresholds)
    inter = R.intersections(gt, m[sel])
    table = inter / (gt.sum(1)[:, None] + m[sel].sum(1)[None, :] - inter)
    assert np.array_equal(out["best_iou"], table.max(1))
    assert np.array_equal(out["recall"], [(table.max(1) >= t).mean() for t in thresholds])
    assert 0.0 < out["recall"][0] and out["recall"][3] < 1.0
    empty = Proposals(N, prop.bits[:0], prop.candidate[:0], prop.prompt_index[:0], z[:0], prop.area[:0], z[:0], prop.labels)
    assert (proposal_recall(empty, torch.from_numpy(gt), thresholds)["recall"] == 0.0).all()


def test_segment_all_route_on_a_real_model(ops):
    from point_sam_amd.demo_server import DemoSession, serve
    from point_sam_amd.model import PointCloudSAM
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    pred = PointSAMPredictor(PointCloudSAM(cfg, random_state_dict(cfg, 3), "cuda", precision="f16x3"))
    sess = DemoSession(pred)
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def req(path, body):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=120)
        c.request("POST", path, json.dumps(body), {"Content-Type": "application/json"})
        r = c.getresponse()
        return r.status, json.loads(r.read())

    try:
        xyz, rgb, _, _ = O.synthetic_batch(1, 2048, seed=8)
        st, _ = req("/sampled_pointcloud", {"points": {str(i): float(v) for i, v in enumerate(xyz.flatten().tolist())},
                                            "colors": {str(i): float(v) for i, v in enumerate(rgb.flatten().tolist())}})
        assert st == 200
        st, out = req("/segment_all", {"num_prompts": 32, "prompt_chunk": 16, "mask_threshold": 1.5, "pred_iou_thresh": -1e30, "stability_thresh": 0.0,
                                       "min_points": 1, "max_area_frac": 1.0001})
        assert st == 200, out
        k = out["num_masks"]
        assert len(out["labels"]) == 2048 and len(out["scores"]) == k and k >= 1
        assert all(isinstance(v, int) and -1 <= v < k for v in out["labels"]) and 0 in out["labels"]
        assert out["scores"] == sorted(out["scores"], reverse=True)
        st, out = req("/segment_all", {"threshold": 0.0})
        assert st == 400 and "unknown" in out["error"]
    finally:
        srv.shutdown()
