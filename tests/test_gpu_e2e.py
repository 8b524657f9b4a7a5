"""End-to-end parity of the HIP path (through the reference-shaped host interface) against
  (a) the golden vectors produced by the reference's own modules (tests/golden), and
  (b) the CPU oracle on the same seeded inputs, up to BASELINE.json's full single-cloud size (ViT-L, N=32768, 512x64),
plus size-independent properties (determinism, batch independence, click-loop cache consistency).
Tolerance: north_star's 1e-3 on mask logits (fp32); FPS / kNN / 3-NN indices bit-exact."""
from dataclasses import replace

import pytest
import torch

from oracle import pointsam_oracle as O
from point_sam_amd.config import VIT_GIANT, ModelConfig, get_config
from point_sam_amd.weights import random_state_dict, state_dict_checksum
from workspace_check import check_exact_workspace

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd.model import PointCloudSAM
    return PointCloudSAM


def _maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def _needs_experiments():
    from point_sam_amd import _lib
    if not _lib.has_experiments():
        pytest.skip("measured-and-rejected path: the library was built without PSAM_BUILD_EXPERIMENTS=1")


@pytest.mark.parametrize("which", ["golden_swiglu", "golden_gelu", "golden_radius", "golden_central"])
def test_against_reference_golden(gpu, which, request):
    meta, a = request.getfixturevalue(which)
    cfg = get_config(meta["cfg"])
    sd = random_state_dict(cfg, seed=meta["seed"])
    assert state_dict_checksum(sd) == pytest.approx(meta["weights_checksum"], rel=1e-12)
    model = gpu(cfg, sd)
    st = model.encode(a["xyz"].cuda(), a["rgb"].cuda())
    assert torch.equal(st.fps_idx.cpu(), a["fps_idx"]), "FPS indices differ from the reference run"
    assert torch.equal(st.centers.cpu(), a["centers"])
    assert torch.equal(st.knn_idx.cpu().sort(-1).values, a["knn_idx"].sort(-1).values), "kNN sets differ from torch.cdist+topk"
    assert _maxerr(st.patch_embeddings, a["patch_embeddings"]) < 1e-4
    assert _maxerr(st.pc_embeddings, a["pc_embeddings"]) < 5e-4
    assert _maxerr(st.pc_pe, a["pc_pe"]) < 5e-5
    masks, iou = model.decode(st, a["prompt_coords"].cuda(), a["prompt_labels"].cuda(), None, True)
    assert masks.shape == a["masks_click1"].shape and iou.shape == a["iou_click1"].shape
    assert _maxerr(masks, a["masks_click1"]) < TOL, _maxerr(masks, a["masks_click1"])
    assert _maxerr(iou, a["iou_click1"]) < TOL
    masks2, iou2 = model.decode(st, a["prompt_coords"].cuda(), a["prompt_labels"].cuda(), a["prompt_masks_click2"].cuda(), False)
    assert _maxerr(masks2, a["masks_click2"]) < TOL, _maxerr(masks2, a["masks_click2"])
    assert _maxerr(iou2, a["iou_click2"]) < TOL
    model.check_coordinate_range()


def _giant_slim():
    return ModelConfig(replace(VIT_GIANT, depth=2), 128, 32)


CASES = {
    # name: (config, B, N, M)
    "cfg1_base_4096_128x32": (lambda: get_config("base", 128, 32), 1, 4096, 1),
    "tiny_ragged": (lambda: get_config("tiny", 37, 11), 3, 1000, 2),
    "giant_width_depth2": (_giant_slim, 1, 3000, 1),
    "cfg2_large_32768_512x64": (lambda: get_config("large", 512, 64), 1, 32768, 1),
}


@pytest.mark.parametrize("precision", ["f32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("name", list(CASES))
def test_against_oracle(gpu, name, precision):
    mk, B, N, M = CASES[name]
    cfg = mk()
    sd = random_state_dict(cfg, seed=42)
    xyz, rgb, prompt, labels = O.synthetic_batch(B, N, seed=42, num_prompts=1)
    prompt = prompt.repeat_interleave(M, 0)
    labels = labels.repeat_interleave(M, 0)
    if M > 1:
        prompt = prompt + 0.0  # same click per mask set is fine: exercises the repeat path
    torch.set_num_threads(max(1, torch.get_num_threads()))
    want_masks, want_iou, mid = O.predict_masks(sd, cfg, xyz, rgb, prompt, labels, None, True, mode="exact", return_intermediates=True)
    model = gpu(cfg, sd, precision=precision)
    st = model.encode(xyz.cuda(), rgb.cuda())
    assert torch.equal(st.fps_idx.cpu(), mid["patches"]["fps_idx"]), "FPS indices not bit-exact"
    assert torch.equal(st.knn_idx.cpu(), mid["patches"]["knn_idx"]), "kNN indices not bit-exact"
    e_emb = _maxerr(st.pc_embeddings, mid["pc_embeddings"])
    masks, iou = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
    assert torch.equal(st.interp_index.cpu(), mid["aux"].interp_index), "3-NN indices not bit-exact"
    e_m, e_i = _maxerr(masks, want_masks), _maxerr(iou, want_iou)
    print(f"\n[{name} {precision}] max|err| embeddings {e_emb:.2e} masks {e_m:.2e} iou {e_i:.2e} (|logit| max {want_masks.abs().max():.2f})")
    assert e_m < TOL and e_i < TOL, (e_emb, e_m, e_i)
    # second click: previous best mask as dense prompt, single-mask output
    best = torch.gather(want_masks, 1, want_iou.argmax(1).view(-1, 1, 1).expand(-1, 1, N))[:, 0]
    want2, want_iou2 = O.mask_decoder(sd, cfg, mid["pc_embeddings"], mid["pc_pe"], mid["sparse"],
                                      O.mask_encoder(sd, cfg, best, xyz, mid["patches"]["centers"], mid["patches"]["knn_idx"]), mid["aux"], False)
    masks2, iou2 = model.decode(st, prompt.cuda(), labels.cuda(), best.cuda(), False)
    assert _maxerr(masks2, want2) < TOL and _maxerr(iou2, want_iou2) < TOL, (_maxerr(masks2, want2), _maxerr(iou2, want_iou2))


def _heavy_tailed(sd, seed, fc1_shift=0.0, gain=15.0, massive=0.0):
    """Trained-checkpoint-like statistics on top of the seeded Gaussians: sparse 30x outlier weights, 1 % of the output rows `gain` x
    (massive-activation channels), 1 % of the input columns 8x, 1 % of the LayerNorm gains `gain` x and offsets of a few units, bias outliers.  What the a-priori
    bounds behind the packed q|k|v / attention-output / SwiGLU scales (Cauchy-Schwarz on weight row norms, max |gamma|) have to survive."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        t = v.clone()
        if "norm" in k and t.dim() == 1:
            hot = torch.rand(t.shape, generator=g) < 0.01
            t = torch.where(hot, t * gain if k.endswith("weight") else t + 3.0 * torch.sign(torch.randn(t.shape, generator=g)), t)
        elif t.dim() == 2 and k.endswith(".weight") and min(t.shape) >= 64:
            t = torch.where(torch.rand(t.shape, generator=g) < 5e-4, t * 30.0, t)
            t = t * torch.where(torch.rand(t.shape[0], 1, generator=g) < 0.01, gain, 1.0)      # output rows: massive-activation channels
            t = t * torch.where(torch.rand(1, t.shape[1], generator=g) < 0.01, 8.0, 1.0)
        elif t.dim() == 1 and k.endswith("bias"):
            t = torch.where(torch.rand(t.shape, generator=g) < 0.01, t + 2.0 * torch.sign(torch.randn(t.shape, generator=g)), t)
        if massive and k.endswith(("mlp.fc2.weight", "attn.proj.weight")) and "pc_encoder.transformer.blocks" in k:
            t[[7, 100]] = t[[7, 100]] * massive      # the same two residual channels in every block: "massive activations" (hundreds of times the rest)
        if fc1_shift and k.endswith(("mlp.fc1_g.bias", "mlp.fc1_x.bias")):
            t = t + fc1_shift      # gated rows u = silu(g) x with mean >> std: the LayerNorm folded into fc2 (rstd (u.W2g - mean c)) cancels digits
        out[k] = t.contiguous()
    return out


@pytest.mark.parametrize("name,B,fc1_shift,gain,massive", [("base", 2, 0.0, 15.0, 0.0), ("large_slim", 2, 20.0, 15.0, 0.0), ("large", 2, 0.0, 50.0, 0.0),
                                                           ("giant_slim", 4, 0.0, 30.0, 0.0), ("large_slim", 2, 0.0, 15.0, 300.0), ("base", 2, 0.0, 1.0, 1000.0)])
def test_heavy_tailed_weights_against_oracle(gpu, name, B, fc1_shift, gain, massive):
    """Robustness of the bound-derived fp16 scales (packed q|k|v with ONE a-priori scale, packed attention output, SwiGLU rows, folded
    LayerNorm) under trained-checkpoint-like weight statistics: nothing overflows fp16 (finite outputs), and the f16x3 path stays as close
    to the oracle as the exact-fp32-product path does (logits here are 10-100x those of Gaussian weights, so the bar is relative)."""
    cfg = {"large_slim": lambda: ModelConfig(replace(get_config("large", 128, 32).vit, depth=4), 128, 32), "giant_slim": _giant_slim}.get(
        name, lambda: get_config(name, 128, 32))()
    sd = _heavy_tailed(random_state_dict(cfg, seed=11), seed=12, fc1_shift=fc1_shift, gain=gain, massive=massive)
    xyz, rgb, prompt, labels = O.synthetic_batch(B, 4096, seed=13, num_prompts=1)
    want_masks, want_iou, mid = O.predict_masks(sd, cfg, xyz, rgb, prompt, labels, None, True, mode="exact", return_intermediates=True)
    scale = max(1.0, want_masks.abs().max().item())
    errs = {}
    for precision in ("f32", "f16x3"):
        model = gpu(cfg, sd, precision=precision)
        st = model.encode(xyz.cuda(), rgb.cuda())
        assert torch.equal(st.fps_idx.cpu(), mid["patches"]["fps_idx"]) and torch.equal(st.knn_idx.cpu(), mid["patches"]["knn_idx"])
        masks, iou = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
        assert torch.isfinite(masks).all() and torch.isfinite(iou).all() and torch.isfinite(st.pc_embeddings).all(), precision
        errs[precision] = (_maxerr(st.pc_embeddings, mid["pc_embeddings"]), _maxerr(masks, want_masks), _maxerr(iou, want_iou))
    print(f"\n[heavy-tailed {name} gain {gain} fc1 bias shift {fc1_shift} massive x{massive}] |logit| max {scale:.1f}, |emb| max {mid['pc_embeddings'].abs().max():.1f}; max|err| (emb, masks, iou) "
          f"f32 {errs['f32'][0]:.2e} {errs['f32'][1]:.2e} {errs['f32'][2]:.2e} | f16x3 {errs['f16x3'][0]:.2e} {errs['f16x3'][1]:.2e} {errs['f16x3'][2]:.2e}")
    assert errs["f16x3"][1] < TOL * scale and errs["f16x3"][2] < TOL * max(1.0, want_iou.abs().max().item())
    assert errs["f16x3"][1] < 4 * errs["f32"][1] + 1e-5 * scale, errs


@pytest.mark.parametrize("precision,B,clicks,rep", [("f32", 2, 1, 1), ("f16x3", 2, 3, 2), ("f16x3", 1, 9, 1)])
def test_fused_token_decoder_matches_unfused(gpu, precision, B, clicks, rep):
    """One launch per two-way layer for the token side (csrc/experiments/twoway.hip: team of workgroups, counter barriers between the stages) against the
    ~22 separate launches it replaces: same arithmetic, so the logits agree to fp32 round-off; repeated runs are bitwise equal (no stage reads
    a row before the barrier that publishes it); with and without a dense prompt mask."""
    _needs_experiments()
    cfg = get_config("base", 128, 32)
    sd = random_state_dict(cfg, seed=5)
    xyz, rgb, prompt, labels = O.synthetic_batch(B, 4096, seed=21, num_prompts=clicks)
    prompt, labels = prompt.repeat_interleave(rep, 0).cuda(), labels.repeat_interleave(rep, 0).cuda()
    model = gpu(cfg, sd, precision=precision)
    st = model.encode(xyz.cuda(), rgb.cuda())
    outs = {}
    for fuse in (True, False):
        model.fuse_tokens = fuse
        m1, i1 = model.decode(st, prompt, labels, None, True)
        best = torch.gather(m1, 1, i1.argmax(1).view(-1, 1, 1).expand(-1, 1, m1.shape[2]))[:, 0]
        m2, i2 = model.decode(st, prompt, labels, best, False)
        outs[fuse] = (m1, i1, m2, i2)
        if fuse:
            for _ in range(3):
                again = model.decode(st, prompt, labels, None, True)
                assert torch.equal(again[0], m1) and torch.equal(again[1], i1)
    errs = [_maxerr(a, b) for a, b in zip(outs[True], outs[False])]
    print(f"\n[token kernel vs separate launches, {precision}, Z={B * rep}, T={5 + clicks}] max|diff| {errs}")
    assert max(errs) < 2e-5, errs


def test_c_eva_block_matches_python_sequence(gpu):
    """psam_eva_block (csrc/blocks.hip: the library packs a block's weights and sequences its eight launches) against the same launches sequenced by
    the Python host from its own packing: the kernels and their order are the same, the bounds are computed twice (C++ doubles / torch doubles), so the
    embeddings agree to fp32 round-off at worst; also directly through the C ABI on one block."""
    from point_sam_amd import ops
    cfg = get_config("base", 128, 32)
    sd = random_state_dict(cfg, seed=8)
    xyz, rgb, prompt, labels = O.synthetic_batch(2, 4096, seed=9)
    model = gpu(cfg, sd, precision="f16x3")
    assert all(hasattr(b, "c_block") for b in model.blocks)
    outs = {}
    assert set(model.c_patch) == {"pc_encoder.patch_embed.patch_encoder", "mask_encoder.patch_encoder"} and model.c_upscale is not None
    for c in (True, False):      # c_blocks also switches psam_patch_encoder (patch embedding, mask encoder) and psam_upscale_masks
        model.c_blocks = c
        st = model.encode(xyz.cuda(), rgb.cuda())
        m1, i1 = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
        best = torch.gather(m1, 1, i1.argmax(1).view(-1, 1, 1).expand(-1, 1, m1.shape[2]))[:, 0]
        outs[c] = (st.patch_embeddings, st.pc_embeddings, m1, i1, *model.decode(st, prompt.cuda(), labels.cuda(), best, False))
    errs = [_maxerr(a, b) for a, b in zip(outs[True], outs[False])]
    print(f"\n[coarse C-ABI entries vs Python-sequenced launches, ViT-B x12] max|diff| patch emb {errs[0]:.2e} embeddings {errs[1]:.2e} click1 {errs[2]:.2e} "
          f"{errs[3]:.2e} click2 {errs[4]:.2e} {errs[5]:.2e}")
    # (round 5: the coarse decoder entries regroup their launches and run the few-hundred-row Linears of one cloud on the exact-fp32 row kernel where the
    # Python sequence runs packed-operand GEMMs -- other kernels, other summation orders; both sit 1e-5 from the oracle)
    assert max(errs[:2]) < 2e-5 and max(errs) < 1e-4
    # one block alone, bitwise repeatable, workspace too small refused
    blk = model.blocks[0].c_block
    x = torch.randn(256, cfg.vit.dim, device="cuda")
    a, b = blk.run(x.clone(), 2, 128), blk.run(x.clone(), 2, 128)
    assert torch.equal(a, b) and torch.isfinite(a).all() and not torch.equal(a, x)
    import ctypes
    lib = ops._lib.load()
    small = torch.empty(1024, dtype=torch.uint8, device="cuda")
    assert lib.psam_eva_block(ctypes.byref(blk.plan), blk.blob.data_ptr(), x.data_ptr(), 2, 128, small.data_ptr(), small.numel(), None) == -3      # PSAM_EWORKSPACE
    with pytest.raises(Exception):
        blk.run(torch.randn(100, cfg.vit.dim, device="cuda"), 1, 100)      # M % 256 != 0


def test_twoway_decoder_fork_is_bitwise_equal_to_serial(gpu):
    """psam_twoway_decoder issues the patch-side projections of each layer (keys + key_pe packed, k / v for token -> patch, q for patch -> token) on a side
    stream forked from the caller's stream and joins them where they are consumed.  Same kernels on the same data: the logits must be the SAME BITS as
    with everything in sequence on one stream -- first click (no mask prompt) and a second click with the mask prompt, several prompt sets per cloud."""
    _needs_experiments()
    from point_sam_amd import ops
    L = ops._lib.load()
    cfg = get_config("base", 256, 32)
    sd = random_state_dict(cfg, seed=18)
    xyz, rgb, prompt, labels = O.synthetic_batch(2, 8192, seed=19, num_prompts=3)
    model = gpu(cfg, sd, precision="f16x3")
    assert model.c_twoway is not None
    st = model.encode(xyz.cuda(), rgb.cuda())
    outs = {}
    try:
        L.psam_twoway_decoder_force_fast(0)      # the fork exists in the operator-by-operator sequence only (the regrouped sequence has no side chain left to fork)
        for mode in (0, 1, 0, 1):
            L.psam_twoway_decoder_force_fork(mode)
            m1, i1 = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
            best = torch.gather(m1, 1, i1.argmax(1).view(-1, 1, 1).expand(-1, 1, m1.shape[2]))[:, 0]
            m2, i2 = model.decode(st, prompt.cuda(), labels.cuda(), best, False)
            torch.cuda.synchronize()
            got = (m1, i1, m2, i2)
            if mode in outs:
                assert all(torch.equal(a, b) for a, b in zip(outs[mode], got)), f"fork={mode}: not repeatable"
            outs[mode] = got
    finally:
        L.psam_twoway_decoder_force_fork(-1)
        L.psam_twoway_decoder_force_fast(-1)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


@pytest.mark.parametrize("B,G,num_prompts", [(1, 512, 1), (2, 256, 3), (1, 1024, 2)])
def test_twoway_decoder_regrouped_sequence_matches_operator_sequence(gpu, B, G, num_prompts):
    """psam_twoway_decoder's regrouped launch sequence (round 5: Linear + residual + LayerNorm of the token side in one launch each, lin2 split over K,
    the projections of the finished queries in one launch, both packed forms of the keys in one pass, [k | q] of the patch side as one GEMM) against
    its operator-by-operator sequence (what the Python host issues; transformer.py:61-176): a first click and a second one with the mask prompt and
    more points, logits and IoU to fp32 round-off; the regrouped sequence repeatable bit for bit; both against the oracle."""
    from point_sam_amd import ops
    L = ops._lib.load()
    cfg = get_config("base", G, 32)
    sd = random_state_dict(cfg, seed=28)
    xyz, rgb, prompt, labels = O.synthetic_batch(B, 8192, seed=29, num_prompts=num_prompts)
    model = gpu(cfg, sd, precision="f16x3")
    assert model.c_twoway is not None
    st = model.encode(xyz.cuda(), rgb.cuda())
    Z = prompt.shape[0]
    extra = xyz[torch.arange(Z) // (Z // B), :2]
    pc2, pl2 = torch.cat([prompt, extra], 1).cuda(), torch.ones(Z, prompt.shape[1] + 2, dtype=labels.dtype, device="cuda")
    outs = {}
    try:
        for mode in (0, 1, 2, 2):      # operator sequence; regrouped with packed-operand GEMMs on the patch side; regrouped with the exact-fp32 row kernel (default), twice
            L.psam_twoway_decoder_force_fast(mode)
            m1, i1 = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
            best = torch.gather(m1, 1, i1.argmax(1).view(-1, 1, 1).expand(-1, 1, m1.shape[2]))[:, 0] if mode == 0 else outs[0][4]
            m2, i2 = model.decode(st, pc2, pl2, best, False)
            torch.cuda.synchronize()
            got = (m1, i1, m2, i2, best)
            if mode in outs:
                assert all(torch.equal(a, b) for a, b in zip(outs[mode], got)), "regrouped sequence: not repeatable"
            outs[mode] = got
    finally:
        L.psam_twoway_decoder_force_fast(-1)
    want_m, want_i = O.predict_masks(sd, cfg, xyz, rgb, prompt, labels, None, True, mode="exact")
    for mode in (1, 2):
        errs = [_maxerr(a, b) for a, b in zip(outs[0][:4], outs[mode][:4])]
        print(f"\n[two-way decoder, regrouped (mode {mode}) vs operator sequence, Z={Z} G={G}] max|diff| click1 {errs[0]:.2e} {errs[1]:.2e} click2 {errs[2]:.2e} {errs[3]:.2e}")
        assert max(errs) < 1e-4, errs
        assert _maxerr(outs[mode][0], want_m) < 1e-3 and _maxerr(outs[mode][1], want_i) < 1e-3


def test_c_eva_gelu_block_matches_python_sequence(gpu):
    """psam_eva_gelu_block (the giant encoder's block through the coarse C ABI: fused qkv with q / v bias, head dim 88 on the fp16-pipe attention,
    GELU MLP, the library's split-K factors) against the same launches sequenced by the Python host: one cloud (M = 512 token rows: split-K in
    every plain GEMM, fc1 unfused) and a batch (M = 2304: no split, fc1 hands GELU(.) to fc2 packed) -- the same kernels in the same order with
    the same decisions, so the embeddings agree to fp32 round-off at worst (the bounds are computed twice: C++ doubles / torch doubles)."""
    from dataclasses import replace
    from point_sam_amd import ops
    from point_sam_amd.config import ViTConfig
    cfg = replace(get_config("giant", 256, 16), vit=ViTConfig("mini_eva_giant", 352, 3, 4, 1024, False))      # head dim 88
    sd = random_state_dict(cfg, seed=12)
    model = gpu(cfg, sd, precision="f16x3")
    assert all(isinstance(b.c_block, ops.EvaGeluBlock) for b in model.blocks)
    for B, N in ((2, 4096), (9, 2048)):
        xyz, rgb, prompt, labels = O.synthetic_batch(B, N, seed=13 + B)
        outs = {}
        for c in (True, False):
            model.c_blocks = c
            st = model.encode(xyz.cuda(), rgb.cuda())
            outs[c] = (st.pc_embeddings, *model.decode(st, prompt.cuda(), labels.cuda(), None, True))
        model.c_blocks = True
        errs = [_maxerr(a, b) for a, b in zip(outs[True], outs[False])]
        print(f"\n[psam_eva_gelu_block vs Python-sequenced launches, B={B} (M={B * 256})] max|diff| embeddings {errs[0]:.2e} masks {errs[1]:.2e} iou {errs[2]:.2e}")
        assert max(errs) < 2e-5
    blk = model.blocks[0].c_block
    x = torch.randn(512, cfg.vit.dim, device="cuda")
    a, b = blk.run(x.clone(), 2, 256), blk.run(x.clone(), 2, 256)
    assert torch.equal(a, b) and torch.isfinite(a).all() and not torch.equal(a, x)
    import ctypes
    lib = ops._lib.load()
    small = torch.empty(1024, dtype=torch.uint8, device="cuda")
    assert lib.psam_eva_gelu_block(ctypes.byref(blk.plan), blk.blob.data_ptr(), x.data_ptr(), 2, 256, small.data_ptr(), small.numel(), None, None) == -3      # PSAM_EWORKSPACE


def _record_runs(stage):
    """Every later stage.run(...) also leaves (args, kwargs) in the returned list, tensors cloned before the call."""
    calls, run = [], stage.run
    keep = lambda v: v.clone() if torch.is_tensor(v) else v

    def recording(*args, **kwargs):
        calls.append((tuple(keep(v) for v in args), {k: keep(v) for k, v in kwargs.items()}))
        return run(*args, **kwargs)
    stage.run = recording
    return calls


@pytest.mark.parametrize("kind,B,L", [("swiglu", 2, 128), ("gelu", 2, 256), ("gelu", 9, 256)])
def test_exact_workspace_of_the_encoder_blocks(gpu, kind, B, L):
    """psam_eva_block (block 0 of ViT-B) and psam_eva_gelu_block (the mini giant block: one cloud, M = 512, split-K planes and counters in use; a batch,
    M = 2304, the fused GELU hand-over) on a workspace of exactly *_ws_bytes (check_exact_workspace)."""
    import ctypes
    from point_sam_amd import ops
    from point_sam_amd.config import ViTConfig
    lib = ops._lib.load()
    cfg = get_config("base", 128, 32) if kind == "swiglu" else replace(get_config("giant", 256, 16), vit=ViTConfig("mini_eva_giant", 352, 3, 4, 1024, False))
    blk = gpu(cfg, random_state_dict(cfg, seed=8), precision="f16x3").blocks[0].c_block
    assert isinstance(blk, ops.EvaBlock if kind == "swiglu" else ops.EvaGeluBlock)
    x0 = torch.randn(B * L, cfg.vit.dim, device="cuda")
    x, want = x0.clone(), blk.run(x0.clone(), B, L)
    assert torch.isfinite(want).all() and not torch.equal(want, x0)
    if kind == "swiglu":
        need = lib.psam_eva_block_ws_bytes(B * L, blk.dim, blk.hidden)
        call = lambda ws, n: lib.psam_eva_block(ctypes.byref(blk.plan), blk.blob.data_ptr(), x.data_ptr(), B, L, ws, n, ops._stream())
    else:
        need = lib.psam_eva_gelu_block_ws_bytes(B * L, blk.dim, blk.hidden)
        counters = ops.arrival_counters(x.device)
        call = lambda ws, n: lib.psam_eva_gelu_block(ctypes.byref(blk.plan), blk.blob.data_ptr(), x.data_ptr(), B, L, ws, n, counters.data_ptr(), ops._stream())
    check_exact_workspace(need, call, lambda: x.copy_(x0), lambda: [x], [want])


@pytest.mark.parametrize("G,K", [(128, 64), (32, 256)])
def test_exact_workspace_of_the_patch_encoder(gpu, G, K):
    """psam_patch_encoder as the patch embedding calls it, groups of 64 and of 256 (pooled in 64-row parts: the partial maxima reuse two buffers of the
    workspace), on a workspace of exactly psam_patch_encoder_ws_bytes (check_exact_workspace)."""
    import ctypes
    from point_sam_amd import ops
    lib = ops._lib.load()
    cfg = get_config("tiny", G, K)
    model = gpu(cfg, random_state_dict(cfg, seed=3), precision="f16x3")
    enc = model.c_patch["pc_encoder.patch_embed.patch_encoder"]
    calls = _record_runs(enc)
    xyz, rgb, _, _ = O.synthetic_batch(2, 9000, seed=4)
    model.encode(xyz.cuda(), rgb.cuda())
    (pts, feats, centers, knn_idx), kw = calls[0]
    want = enc.run(pts, feats, centers, knn_idx, **kw)
    B, N, rep = pts.shape[0], pts.shape[1], feats.shape[0] // pts.shape[0]
    groups = B * rep * G
    assert tuple(knn_idx.shape[1:]) == (G, K) and want.shape == (groups, enc.cout) and torch.isfinite(want).all()
    out = torch.empty_like(want)
    call = lambda ws, n: lib.psam_patch_encoder(ctypes.byref(enc.plan), enc.blob.data_ptr(), pts.data_ptr(), feats.data_ptr(), centers.data_ptr(), knn_idx.data_ptr(),
                                                ops._p(kw.get("center_idx")), B, rep, N, G, K, feats.shape[-1], float(kw.get("radius") or 0.0), out.data_ptr(), ws, n,
                                                ops._stream())
    check_exact_workspace(lib.psam_patch_encoder_ws_bytes(groups * K, groups, enc.h0, enc.h1), call, lambda: out.fill_(-7.0), lambda: [out], [want])


def test_exact_workspace_of_the_upscaling(gpu):
    """psam_upscale_masks as the decoder calls it on a workspace of exactly psam_upscale_masks_ws_bytes (check_exact_workspace)."""
    import ctypes
    from point_sam_amd import ops
    lib = ops._lib.load()
    cfg = get_config("tiny", 64, 16)
    model = gpu(cfg, random_state_dict(cfg, seed=8), precision="f16x3")
    up = model.c_upscale
    calls = _record_runs(up)
    xyz, rgb, prompt, labels = O.synthetic_batch(2, 4096, seed=5)
    model.predict_masks(xyz.cuda(), rgb.cuda(), prompt.cuda(), labels.cuda())
    (keys, idx3, w3, hyper, masks, rep, Z, N, G, C), _ = calls[0]
    want = up.run(keys, idx3, w3, hyper, torch.empty_like(masks), rep, Z, N, G, C)
    assert (N, G) == (4096, 64) and torch.isfinite(want).all()
    call = lambda ws, n: lib.psam_upscale_masks(ctypes.byref(up.plan), up.blob.data_ptr(), keys.data_ptr(), idx3.data_ptr(), w3.data_ptr(), hyper.data_ptr(), rep, Z, N, G, C,
                                                masks.data_ptr(), ws, n, ops._stream())
    check_exact_workspace(lib.psam_upscale_masks_ws_bytes(Z, N, G, C, up.dim), call, lambda: masks.fill_(-7.0), lambda: [masks], [want])


def test_exact_workspace_of_the_twoway_decoder(gpu):
    """psam_twoway_decoder as the decoder calls it (two clouds, three prompt points each) on a workspace of exactly psam_twoway_decoder_ws_bytes
    (check_exact_workspace), in each of its three launch sequences: they use different buffers of the workspace."""
    import ctypes
    from point_sam_amd import ops
    lib = ops._lib.load()
    cfg = get_config("base", 256, 32)
    model = gpu(cfg, random_state_dict(cfg, seed=18), precision="f16x3")
    tw = model.c_twoway
    calls = _record_runs(tw)
    xyz, rgb, prompt, labels = O.synthetic_batch(2, 8192, seed=19, num_prompts=3)
    model.predict_masks(xyz.cuda(), rgb.cuda(), prompt.cuda(), labels.cuda())
    (tokens, keys0, pos, rep, Z, T, G), _ = calls[0]
    assert (Z, G) == (2, 256) and T > 3
    keys, queries = keys0.clone(), torch.empty(Z * T, tw.dim, device="cuda")
    counters = ops.arrival_counters(tokens.device)
    call = lambda ws, n: lib.psam_twoway_decoder(ctypes.byref(tw.plan), tw.blob.data_ptr(), tokens.data_ptr(), keys.data_ptr(), pos.data_ptr(), rep, Z, T, G, queries.data_ptr(),
                                                 ws, n, counters.data_ptr(), ops._stream())

    def reset():
        keys.copy_(keys0)
        queries.fill_(-7.0)
    try:
        for mode in (0, 1, 2):
            lib.psam_twoway_decoder_force_fast(mode)
            want = tw.run(tokens, keys0.clone(), pos, rep, Z, T, G)
            assert all(torch.isfinite(t).all() for t in want) and not torch.equal(want[1], keys0)
            check_exact_workspace(lib.psam_twoway_decoder_ws_bytes(Z, T, G, tw.dim, tw.mlp), call, reset, lambda: [queries, keys], list(want))
    finally:
        lib.psam_twoway_decoder_force_fast(-1)


def test_attention_packed_output_is_transparent(gpu):
    """Attention writing its output packed for the projection (bound-derived per-cloud scale) vs fp32 output + separate pack pass: a
    power-of-two scale does not change the decoded hi + lo except where lo goes subnormal (elements ~2^-10 below the row maximum, since
    the bound sits a few binades above the actual outputs): the model outputs agree to fp32 round-off."""
    cfg = get_config("base", 128, 32)
    sd = random_state_dict(cfg, seed=2)
    xyz, rgb, prompt, labels = O.synthetic_batch(2, 4096, seed=6)
    outs = []
    for fuse in (True, False):
        model = gpu(cfg, sd, precision="f16x3")
        model.fuse_attn_pack = fuse
        outs.append(model.predict_masks(xyz.cuda(), rgb.cuda(), prompt.cuda(), labels.cuda()))
    e_m, e_i = _maxerr(outs[0][0], outs[1][0]), _maxerr(outs[0][1], outs[1][1])
    print(f"\n[packed attention output vs fp32 + pack pass, ViT-B x12] max|diff| masks {e_m:.2e} iou {e_i:.2e}")
    assert e_m < 5e-5 and e_i < 5e-5


def test_attention_packed_operands_is_transparent(gpu):
    """The qkv GEMM writing q | k | v packed with an a-priori scale + the packed-operand attention kernel, against the fp32 qkv buffer + the
    kernel that converts per tile: the model outputs agree to fp32 round-off (ViT-B: 12 blocks; ViT-L at cfg #2 is covered by
    test_against_oracle, which runs the default = packed path)."""
    cfg = get_config("base", 128, 32)
    sd = random_state_dict(cfg, seed=2)
    xyz, rgb, prompt, labels = O.synthetic_batch(2, 4096, seed=6)
    outs = []
    for fuse in (True, False):
        model = gpu(cfg, sd, precision="f16x3")
        model.fuse_attn_operands = fuse
        outs.append(model.predict_masks(xyz.cuda(), rgb.cuda(), prompt.cuda(), labels.cuda()))
    e_m, e_i = _maxerr(outs[0][0], outs[1][0]), _maxerr(outs[0][1], outs[1][1])
    print(f"\n[packed-operand attention vs per-tile conversion, ViT-B x12] max|diff| masks {e_m:.2e} iou {e_i:.2e}")
    assert e_m < 5e-5 and e_i < 5e-5


def test_fused_upscaling_matches_unfused(gpu):
    """Decoder upscaling chain with the packed interpolation hand-over, and in three kernels (+ row LayerNorm + GELU + re-pack and the
    hyper-network products in GEMM epilogues), vs the six-kernel sequence; multimask and single-mask outputs."""
    cfg = get_config("tiny", 64, 16)
    sd = random_state_dict(cfg, seed=8)
    xyz, rgb, prompt, labels = O.synthetic_batch(2, 4096, seed=5)
    outs = []
    for first, fuse, rows, hyp in ((False, False, False, False), (False, True, False, False), (False, True, True, False), (True, True, False, False),
                                   (True, True, False, True)):
        model = gpu(cfg, sd, precision="f16x3")
        model.upscale_linear_first, model.fuse_upscale, model.fuse_upscale_rows, model.fuse_hyper = first, fuse, rows, hyp
        st = model.encode(xyz.cuda(), rgb.cuda())
        m1, i1 = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
        m2, i2 = model.decode(st, prompt.cuda(), labels.cuda(), m1[:, 1].contiguous(), False)
        outs.append((m1, i1, m2, i2))
    for tag, got in (("packed interpolation", outs[1]), ("row epilogues", outs[2]), ("Linear before interpolation + LN/GELU in the interpolation kernel", outs[3]),
                     ("... + hyper products in the GEMM epilogue", outs[4])):
        e = [_maxerr(a, b) for a, b in zip(outs[0], got)]
        print(f"\n[upscaling: {tag} vs unfused] max|diff| masks {e[0]:.2e} iou {e[1]:.2e} click-2 masks {e[2]:.2e}")
        assert max(e) < 5e-5, e


def test_fused_mlp_matches_unfused_model(gpu):
    """The two-GEMM MLP (inner LayerNorm folded into fc2, packed hand-over) vs the three-kernel sequence on a whole ViT-L stack."""
    cfg = get_config("large", 256, 32)
    sd = random_state_dict(cfg, seed=42)
    xyz, rgb, prompt, labels = O.synthetic_batch(1, 8192, seed=6)
    outs = []
    for fuse in (True, False):
        model = gpu(cfg, sd, precision="f16x3")
        model.fuse_mlp = fuse
        st = model.encode(xyz.cuda(), rgb.cuda())
        masks, iou = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
        outs.append((st.pc_embeddings, masks, iou))
    e_emb, e_m = _maxerr(outs[0][0], outs[1][0]), _maxerr(outs[0][1], outs[1][1])
    print(f"\n[fused vs unfused MLP, ViT-L x24] max|diff| embeddings {e_emb:.2e} masks {e_m:.2e}")
    assert e_emb < 1e-4 and e_m < 1e-4


def test_fused_patch_encoder_matches_unfused(gpu):
    """Mini-PointNet with packed hand-overs and the two max-pools inside GEMM epilogues vs the separate-kernel sequence, for the point
    patch encoder (6 input channels) and the mask encoder (4 channels, second click), groups of 64 and of 32, and of 128 / 256 (pooled as 64-row
    parts in the epilogues + a small pass over the parts: cfg #3's group size); the fused form through psam_patch_encoder and sequenced by the host."""
    for G, K, c_blocks in ((128, 64, True), (256, 32, True), (64, 128, True), (32, 256, False), (32, 256, True)):
        cfg = get_config("tiny", G, K)
        sd = random_state_dict(cfg, seed=3)
        xyz, rgb, prompt, labels = O.synthetic_batch(2, 9000, seed=4)
        outs = []
        for fuse in (True, False):
            model = gpu(cfg, sd, precision="f16x3")
            model.fuse_patch, model.c_blocks = fuse, c_blocks
            st = model.encode(xyz.cuda(), rgb.cuda())
            m1, i1 = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
            m2, i2 = model.decode(st, prompt.cuda(), labels.cuda(), m1[:, 0].contiguous(), False)
            outs.append((st.patch_embeddings, m1, m2))
        e = [_maxerr(a, b) for a, b in zip(*outs)]
        print(f"\n[fused vs unfused patch encoder G={G} K={K}] max|diff| patch embeddings {e[0]:.2e} masks {e[1]:.2e} click-2 masks {e[2]:.2e}")
        assert max(e) < 5e-5, e


def test_mask_encoder_centralize_in_forward(gpu):
    """MaskEncoder.centralize_features (logit minus the centre point's logit, common.py:183-186): only reachable through
    PointCloudSAM.forward, which passes center_idx (pc_sam.py:151-157); predict_masks raises as the reference would fail."""
    from dataclasses import replace as dc_replace
    cfg = dc_replace(get_config("tiny"), mask_centralize_features=True, mask_radius=0.3)
    sd = random_state_dict(cfg, seed=12)
    xyz, rgb, prompt, labels = O.synthetic_batch(2, 700, seed=3)
    gt = torch.stack([xyz[..., 0] > 0.1, xyz[..., 2] < -0.2], 1)
    want = O.forward_eval(sd, cfg, xyz, rgb, gt, prompt_iters=3)
    model = gpu(cfg, sd)
    model.prompt_iters = 3
    outs = model(xyz.cuda(), rgb.cuda(), gt.cuda(), is_eval=True)
    for o, w in zip(outs, want):
        assert torch.equal(o["prompt_coords"].cpu(), w["prompt_coords"])
        assert _maxerr(o["masks"], w["masks"]) < TOL and _maxerr(o["iou_preds"], w["iou_preds"]) < TOL
    with pytest.raises(ValueError):
        model.predict_masks(xyz.cuda(), rgb.cuda(), prompt.cuda(), labels.cuda(), prompt_masks=outs[0]["prompt_masks"][:2])


def test_properties_full_size(gpu):
    """BASELINE sizes without an oracle run: determinism and batch independence (clouds never interact)."""
    cfg = get_config("tiny", 512, 64)
    model = gpu(cfg, random_state_dict(cfg, 1))
    xyz, rgb, prompt, labels = O.synthetic_batch(3, 32768, seed=5)
    xyz, rgb, prompt, labels = xyz.cuda(), rgb.cuda(), prompt.cuda(), labels.cuda()
    m1, i1 = model.predict_masks(xyz, rgb, prompt, labels)
    m2, i2 = model.predict_masks(xyz, rgb, prompt, labels)
    assert torch.equal(m1, m2) and torch.equal(i1, i2), "same input twice must be bit-identical"
    ms, _ = model.predict_masks(xyz[1:2].contiguous(), rgb[1:2].contiguous(), prompt[1:2].contiguous(), labels[1:2].contiguous())
    assert torch.equal(ms[0], m1[1]), "a cloud's logits must not depend on its batch neighbours"
    st = model.encode(xyz, rgb)
    idx = st.fps_idx.cpu()
    assert (idx[:, 0] == 0).all() and all(len(set(r.tolist())) == 512 for r in idx)
    assert (st.knn_idx[:, :, 0].cpu() == idx).all(), "each center is its own nearest neighbour"
    model.decode(st, prompt, labels)
    assert torch.allclose(st.interp_weight.sum(-1), torch.ones(3, 32768, device="cuda"), atol=1e-6)


def test_batch_independence_across_the_row_kernel_threshold(gpu):
    """the small-row Linears (pooled conv2.0 of the patch / mask encoder, the first upscaling Linear, the decoder's patch-side projections)
    used to pick their arithmetic from the TOTAL row count B * G -- exact-fp32 row kernel up to 2048 rows, packed f16x3 GEMM above -- so a cloud's logits
    differed in the low bits between a batch of 1 and a batch of 8 at G = 512.  The choice is now made from one cloud's rows: bitwise equal, both clicks."""
    cfg = get_config("tiny", 512, 64)
    model = gpu(cfg, random_state_dict(cfg, 1))
    xyz, rgb, prompt, labels = (t.cuda() for t in O.synthetic_batch(8, 8192, seed=9, num_prompts=2))
    m8, i8 = model.predict_masks(xyz, rgb, prompt[:, :1].contiguous(), labels[:, :1].contiguous())
    best = torch.gather(m8, 1, i8.argmax(1).view(-1, 1, 1).expand(-1, 1, m8.shape[2]))[:, 0].contiguous()
    n8, j8 = model.predict_masks(xyz, rgb, prompt, labels, best, False)
    for b in (0, 5):
        one = lambda t: t[b:b + 1].contiguous()
        m1, i1 = model.predict_masks(one(xyz), one(rgb), one(prompt[:, :1]), one(labels[:, :1]))
        assert torch.equal(m1[0], m8[b]) and torch.equal(i1[0], i8[b]), "click 1: a cloud's logits depend on the batch size"
        n1, j1 = model.predict_masks(one(xyz), one(rgb), one(prompt), one(labels), one(best), False)
        assert torch.equal(n1[0], n8[b]) and torch.equal(j1[0], j8[b]), "click 2 (mask prompt): a cloud's logits depend on the batch size"


def test_predictor_click_loop(gpu):
    from point_sam_amd.predictor import PointSAMPredictor
    cfg = get_config("tiny")
    sd = random_state_dict(cfg, 3)
    pred = PointSAMPredictor(gpu(cfg, sd))
    xyz, rgb, _, _ = O.synthetic_batch(1, 1500, seed=8)
    g = torch.Generator().manual_seed(0)
    clicks = xyz[:, torch.randint(0, 1500, (4,), generator=g)]
    labels = torch.tensor([[1, 0, 1, 1]])
    want = O.click_loop(sd, cfg, xyz, rgb, clicks, labels)
    xyz_d, rgb_d = xyz.cuda(), rgb.cuda()
    prompt_mask = None
    for t in range(4):  # demo/app.py:177-206 protocol
        pred.set_pointcloud(xyz_d, rgb_d)
        state_before = pred._state
        mask, scores, logits = pred.predict_masks(clicks[:, : t + 1].cuda(), labels[:, : t + 1].cuda(), prompt_mask, prompt_mask is None)
        assert pred._state is state_before, "encoder must be cached across clicks"
        assert _maxerr(logits, want[t][0]) < TOL and _maxerr(scores, want[t][1]) < TOL, (t, _maxerr(logits, want[t][0]))
        prompt_mask = logits[0][torch.argmax(scores[0])][None, ...]
    pred.set_prompts(clicks[:, :1].cuda(), labels[:, :1].cuda())
    m, s, _ = pred.predict_masks()
    assert _maxerr(m, want[0][0]) < TOL


def test_demo_server_segment_route(gpu):
    """The demo back end (point_sam_amd/demo_server.py) over HTTP on the HIP predictor: /sampled_pointcloud + four /segment
    clicks reproduce the oracle's click loop (demo/app.py:177-206), the encoder runs once."""
    import http.client, json, threading
    from point_sam_amd.predictor import PointSAMPredictor
    from point_sam_amd.demo_server import DemoSession, serve
    cfg = get_config("tiny")
    sd = random_state_dict(cfg, 3)
    pred = PointSAMPredictor(gpu(cfg, sd, precision="f16x3"))
    xyz, rgb, _, _ = O.synthetic_batch(1, 1500, seed=8)
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, 1500, (4,), generator=g)
    labels = [1, 0, 1, 1]
    want = O.click_loop(sd, cfg, xyz, rgb, xyz[:, idx], torch.tensor([labels]))
    sess = DemoSession(pred)
    srv = serve(sess, "127.0.0.1", 0)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        def post(path, body):
            c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=120)
            c.request("POST", path, json.dumps(body), {"Content-Type": "application/json"})
            r = c.getresponse()
            return r.status, json.loads(r.read())
        flat = lambda t: {str(i): float(v) for i, v in enumerate(t.flatten().tolist())}
        assert post("/sampled_pointcloud", {"points": flat(xyz[0]), "colors": flat(rgb[0])}) == (200, {"response": "success"})
        state = None
        for t in range(4):
            st, out = post("/segment", {"prompt_point": xyz[0, idx[t]].tolist(), "prompt_label": labels[t]})
            assert st == 200
            best = want[t][1][0].argmax()
            margin = want[t][0][0, best].abs() > 1e-3                      # ignore points whose logit is within tolerance of 0
            assert torch.equal(torch.tensor(out["seg"])[margin], (want[t][0][0, best] > 0)[margin]), t
            assert _maxerr(sess.prompt_mask, want[t][0][:, best]) < TOL
            state = state or pred._state
            assert pred._state is state, "encoder must be cached across clicks"
        st, out = post("/segment", {"prompt_point": [2.0, 0.0, 0.0], "prompt_label": 1})
        assert st == 400 and "ValueError" in out["error"]                   # prompts outside [-1,1]^3 (prompt_encoder.py:44-46)
    finally:
        srv.shutdown()


def test_out_of_range_coordinates_raise(gpu):
    cfg = get_config("tiny")
    model = gpu(cfg, random_state_dict(cfg, 3))
    xyz, rgb, prompt, labels = O.synthetic_batch(1, 600, seed=2)
    with pytest.raises(ValueError):
        model.predict_masks(xyz.cuda(), rgb.cuda(), (prompt * 0 + 1.5).cuda(), labels.cuda())
    with pytest.raises(AssertionError):
        model.predict_masks(xyz.cuda(), rgb.cuda(), prompt.cuda(), labels[:, :0].cuda())
    m, _ = model.predict_masks(xyz.cuda(), rgb.cuda(), prompt.cuda(), labels.cuda())  # flag was reset
    assert torch.isfinite(m).all()


@pytest.mark.parametrize("dense_streams,precision", [(1, "f32"), (2, "f16x3"), (3, "f16x3")])
def test_batch_pipeline_matches_predict_masks(gpu, dense_streams, precision):
    """The pipeline (tokenizer one batch ahead; optionally several batches in flight on their own dense streams) returns
    bit-identical results to the inline path."""
    from point_sam_amd.model import BatchPipeline
    cfg = get_config("tiny", 64, 16)
    model = gpu(cfg, random_state_dict(cfg, 4), precision=precision)
    batches = []
    for i in range(6):
        xyz, rgb, prompt, labels = O.synthetic_batch(2, 3000 + 500 * i, seed=20 + i)
        batches.append(tuple(t.cuda() for t in (xyz, rgb, prompt, labels)))
    want = [model.predict_masks(*b) for b in batches]
    pipe = BatchPipeline(model, dense_streams=dense_streams)
    got = []
    for k in range(min(pipe.depth, len(batches))):
        pipe.submit(*batches[k])
    for k in range(len(batches)):
        if k + pipe.depth < len(batches):
            pipe.submit(*batches[k + pipe.depth])
        got.append(pipe.next())
    torch.cuda.synchronize()
    for k, ((m1, i1), (m2, i2)) in enumerate(zip(want, got)):
        d = (m1 - m2).abs()
        assert torch.equal(m1, m2) and torch.equal(i1, i2), (k, float(d.max()), [[float(d[z, c].max()) for c in range(d.shape[1])] for z in range(d.shape[0])],
                                                             float((i1 - i2).abs().max()))
    model.check_coordinate_range()


def test_cfg3_large_scene_tokenizer_and_run(gpu):
    """BASELINE config #3 (ViT-L, N=131072, 2048x256, batch 1): the streaming-FPS path, K=256 selection and 3-NN among
    2048 centers are bit-exact against the oracle at full size; the whole path runs and is deterministic."""
    from point_sam_amd import ops
    N, G, K = 131072, 2048, 256
    xyz, rgb, prompt, labels = O.synthetic_batch(1, N, seed=3)
    want_fps = O.fps(xyz, G)
    xyz_d = xyz.cuda()
    idx, centers = ops.fps(xyz_d, G)
    assert torch.equal(idx.cpu(), want_fps)
    sub = torch.arange(0, G, 16)  # every 16th center keeps the C oracle's kNN in seconds
    _, want_knn = O.knn(centers.cpu()[:, sub], xyz, K, "exact")
    got_knn = ops.knn(centers[:, sub].contiguous(), xyz_d, K)
    assert torch.equal(got_knn.cpu(), want_knn)
    wi, ww = O.interp_weights(xyz[:, :8192], centers.cpu(), "exact")
    gi, gw = ops.three_nn(xyz_d[:, :8192].contiguous(), centers)
    assert torch.equal(gi.cpu(), wi) and (gw.cpu() - ww).abs().max() < 1e-6
    cfg = get_config("tiny", G, K)  # full-size tokenizer / grouping / upsampling with a small ViT
    model = gpu(cfg, random_state_dict(cfg, 2), precision="bf16x6")
    m1, i1 = model.predict_masks(xyz_d, rgb.cuda(), prompt.cuda(), labels.cuda())
    m2, i2 = model.predict_masks(xyz_d, rgb.cuda(), prompt.cuda(), labels.cuda())
    assert m1.shape == (1, 3, N) and torch.isfinite(m1).all() and torch.equal(m1, m2)


_CFG5 = {}


def _cfg5_oracle():
    if not _CFG5:
        cfg = get_config("giant", 512, 64)
        sd = random_state_dict(cfg, seed=42)
        N = 32768
        xyz, rgb, _, _ = O.synthetic_batch(1, N, seed=42)
        g = torch.Generator().manual_seed(1)
        clicks = xyz[:, torch.randint(0, N, (5,), generator=g)]
        labels = torch.tensor([[1, 1, 0, 1, 0]])
        _CFG5.update(cfg=cfg, sd=sd, N=N, xyz=xyz, rgb=rgb, clicks=clicks, labels=labels, want=O.click_loop(sd, cfg, xyz, rgb, clicks, labels))
    return _CFG5


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
def test_cfg5_giant_five_click_loop(gpu, precision):
    """BASELINE config #5 (ViT-giant, N=32768, 512x64, 5 clicks, encoder cached) against the oracle's click loop, at the shipped
    default precision ("f16x3": head dim 88 attention included) and at "bf16x6"."""
    from point_sam_amd.predictor import PointSAMPredictor
    c = _cfg5_oracle()
    cfg, sd, N, xyz, rgb, clicks, labels, want = (c[k] for k in ("cfg", "sd", "N", "xyz", "rgb", "clicks", "labels", "want"))
    pred = PointSAMPredictor(gpu(cfg, sd, precision=precision))
    xyz_d, rgb_d = xyz.cuda(), rgb.cuda()
    prompt_mask = None
    for t in range(5):
        pred.set_pointcloud(xyz_d, rgb_d)
        mask, scores, logits = pred.predict_masks(clicks[:, : t + 1].cuda(), labels[:, : t + 1].cuda(), prompt_mask, prompt_mask is None)
        e = _maxerr(logits, want[t][0])
        print(f"\n[giant {precision} click {t + 1}] max|err| {e:.2e}")
        assert e < TOL and _maxerr(scores, want[t][1]) < TOL
        # the oracle feeds ITS best mask forward; do the same so both loops see identical prompts
        wm, wi = want[t]
        prompt_mask = (torch.gather(wm, 1, wi.argmax(1).view(-1, 1, 1).expand(-1, 1, N))[:, 0] if t == 0 else wm[:, 0]).cuda()


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_cfg5_giant_free_running_session(gpu, precision):
    """BASELINE config #5 as the reference runs it (pc_sam.py:139-194): FREE-RUNNING -- every click consumes the model's OWN previous best mask
    (PointCloudSAM.click_session, no teacher forcing), ViT-giant, N = 32768, 512x64, 5 clicks with the bench's label pattern, against the
    oracle's free-running loop.  The error per click is printed for both precisions: the mask-encoder feedback amplifies whatever the first
    click's logits carry, so the growth over the clicks is the number to watch (budget 1e-3)."""
    c = _cfg5_oracle()
    cfg, sd, N, xyz, rgb, clicks, labels, want = (c[k] for k in ("cfg", "sd", "N", "xyz", "rgb", "clicks", "labels", "want"))
    model = gpu(cfg, sd, precision=precision)
    st = model.encode(xyz.cuda(), rgb.cuda())
    outs = model.click_session(st, clicks.cuda(), labels.cuda())
    errs = [(_maxerr(m, wm), _maxerr(i, wi)) for (m, i), (wm, wi) in zip(outs, want)]
    scale = max(float(wm.abs().max()) for wm, _ in want)
    print(f"\n[cfg5 giant free-running {precision}] |logit| max {scale:.2f}; max|err| per click (masks): "
          + " ".join(f"{e[0]:.2e}" for e in errs) + " | (iou): " + " ".join(f"{e[1]:.2e}" for e in errs))
    # the selected candidate of click 1 (the argmax over predicted IoU) must be the oracle's: a flip there would be a different session
    assert int(outs[0][1].argmax(1)) == int(want[0][1].argmax(1))
    for t, (em, ei) in enumerate(errs):
        assert em < TOL and ei < TOL, (precision, t, errs)
    model.check_coordinate_range()


def test_free_running_session_heavy_tailed_weights(gpu):
    """The free-running 5-click loop on trained-checkpoint-like (heavy-tailed) weights at the giant encoder's width: the f16x3 session must stay as
    close to the oracle's free-running loop as the exact-fp32-product session does (bar relative to the logit scale, as in
    test_heavy_tailed_weights_against_oracle)."""
    cfg = _giant_slim()
    sd = _heavy_tailed(random_state_dict(cfg, seed=21), seed=22, gain=30.0)
    N, T = 4096, 5
    xyz, rgb, _, _ = O.synthetic_batch(1, N, seed=23)
    g = torch.Generator().manual_seed(3)
    clicks = xyz[:, torch.randint(0, N, (T,), generator=g)]
    labels = torch.tensor([[1, 1, 0, 1, 0]])
    want = O.click_loop(sd, cfg, xyz, rgb, clicks, labels)
    scale = max(1.0, max(float(wm.abs().max()) for wm, _ in want))
    errs = {}
    for precision in ("f32", "f16x3"):
        model = gpu(cfg, sd, precision=precision)
        outs = model.click_session(model.encode(xyz.cuda(), rgb.cuda()), clicks.cuda(), labels.cuda())
        assert all(torch.isfinite(m).all() and torch.isfinite(i).all() for m, i in outs), precision
        errs[precision] = [_maxerr(m, wm) for (m, _), (wm, _) in zip(outs, want)]
    print(f"\n[free-running heavy-tailed giant-width] |logit| max {scale:.1f}; max|err| per click f32 " + " ".join(f"{e:.2e}" for e in errs["f32"])
          + " | f16x3 " + " ".join(f"{e:.2e}" for e in errs["f16x3"]))
    for t in range(T):
        assert errs["f16x3"][t] < TOL * scale, (t, errs)
        assert errs["f16x3"][t] < 4 * errs["f32"][t] + 2e-5 * scale, (t, errs)


def test_cfg3_gap_to_reference_cdist_mode_is_the_neighbour_sets(gpu):
    """BASELINE config #3 against the reference's OWN kNN arithmetic (torch.cdist's matmul form + topk, pc_sam/model/common.py:51-55): at
    N = 131072 / K = 256 the cdist rounding picks different neighbours for some groups (ties at the K-th distance to ~1e-7), so the HIP
    logits (direct fp32 differences, = oracle mode "exact") differ from mode "reference" by what the swapped neighbours are worth.  That gap
    is a property of the two ORACLE modes, not of the kernels: asserted here as |HIP - reference| <= |exact - reference| + 1e-4, the number
    of differing groups is reported, and on the groups whose sets agree the grouping is bit-identical."""
    cfg = get_config("large", 2048, 256)
    sd = random_state_dict(cfg, seed=42)
    N = 131072
    xyz, rgb, prompt, labels = O.synthetic_batch(1, N, seed=3)
    ex_m, ex_i, ex_mid = O.predict_masks(sd, cfg, xyz, rgb, prompt, labels, None, True, mode="exact", return_intermediates=True)
    rf_m, rf_i, rf_mid = O.predict_masks(sd, cfg, xyz, rgb, prompt, labels, None, True, mode="reference", return_intermediates=True)
    model = gpu(cfg, sd, precision="f16x3")
    st = model.encode(xyz.cuda(), rgb.cuda())
    masks, iou = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
    assert torch.equal(st.fps_idx.cpu(), rf_mid["patches"]["fps_idx"])
    same = (st.knn_idx.cpu().sort(-1).values == rf_mid["patches"]["knn_idx"].sort(-1).values).all(-1)[0]
    assert torch.equal(st.knn_idx.cpu(), ex_mid["patches"]["knn_idx"])
    gap_oracles, gap_hip, err_exact = _maxerr(ex_m, rf_m), _maxerr(masks, rf_m), _maxerr(masks, ex_m)
    print(f"\n[cfg3 vs reference cdist mode] groups whose kNN set differs from cdist+topk: {int((~same).sum())} of {same.numel()}; "
          f"|exact - reference| {gap_oracles:.2e}, |HIP - reference| {gap_hip:.2e}, |HIP - exact| {err_exact:.2e}; iou gaps "
          f"{_maxerr(ex_i, rf_i):.2e} / {_maxerr(iou, rf_i):.2e}")
    assert err_exact < TOL
    assert gap_hip <= gap_oracles + 1e-4 and _maxerr(iou, rf_i) <= _maxerr(ex_i, rf_i) + 1e-4
    if bool(same.all()):      # identical neighbour sets: then the reference-mode logits themselves are within tolerance
        assert gap_hip < TOL


def test_cfg3_large_full_model_vs_oracle(gpu):
    """BASELINE config #3 with the REAL ViT-L (configs/large.yaml geometry of evaluation/eval_kitti.py:352-354: 2048 groups of 256,
    N = 131072, batch 1) at the shipped precision: encoder embeddings (attention over L = 2048 tokens), logits and IoU against the
    oracle; tokenizer indices bit-exact over the whole cloud."""
    cfg = get_config("large", 2048, 256)
    sd = random_state_dict(cfg, seed=42)
    N = 131072
    xyz, rgb, prompt, labels = O.synthetic_batch(1, N, seed=3)
    want_masks, want_iou, mid = O.predict_masks(sd, cfg, xyz, rgb, prompt, labels, None, True, mode="exact", return_intermediates=True)
    model = gpu(cfg, sd, precision="f16x3")
    st = model.encode(xyz.cuda(), rgb.cuda())
    assert torch.equal(st.fps_idx.cpu(), mid["patches"]["fps_idx"]), "FPS indices not bit-exact"
    assert torch.equal(st.knn_idx.cpu(), mid["patches"]["knn_idx"]), "kNN indices not bit-exact"
    masks, iou = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
    model.check_coordinate_range()
    assert torch.equal(st.interp_index.cpu(), mid["aux"].interp_index), "3-NN indices not bit-exact"
    e_emb, e_m, e_i = _maxerr(st.pc_embeddings, mid["pc_embeddings"]), _maxerr(masks, want_masks), _maxerr(iou, want_iou)
    print(f"\n[cfg3 large 131072 2048x256 f16x3] max|err| embeddings {e_emb:.2e} masks {e_m:.2e} iou {e_i:.2e} (|logit| max {want_masks.abs().max():.2f})")
    assert e_emb < TOL and e_m < TOL and e_i < TOL


def test_cfg2_gap_to_reference_cdist_mode(gpu):
    """north_star states the tolerance against the REFERENCE CPU path, whose kNN / 3-NN go through torch.cdist + topk
    (pc_sam/model/common.py:51-55, 238-255) while the HIP kernels use direct fp32 differences.  At BASELINE config #2's full
    single-cloud size: fraction of groups with the identical neighbour set, fraction of points with the identical 3-NN set, and
    the logit gap HIP (shipped precision) vs oracle mode="reference" -- asserted below 1e-3."""
    cfg = get_config("large", 512, 64)
    sd = random_state_dict(cfg, seed=42)
    N = 32768
    xyz, rgb, prompt, labels = O.synthetic_batch(1, N, seed=42)
    ref_masks, ref_iou, mid = O.predict_masks(sd, cfg, xyz, rgb, prompt, labels, None, True, mode="reference", return_intermediates=True)
    model = gpu(cfg, sd, precision="f16x3")
    st = model.encode(xyz.cuda(), rgb.cuda())
    masks, iou = model.decode(st, prompt.cuda(), labels.cuda(), None, True)
    assert torch.equal(st.fps_idx.cpu(), mid["patches"]["fps_idx"])
    knn_same = (st.knn_idx.cpu().sort(-1).values == mid["patches"]["knn_idx"].sort(-1).values).all(-1).float().mean().item()
    nn3_same = (st.interp_index.cpu().sort(-1).values == mid["aux"].interp_index.sort(-1).values).all(-1).float().mean().item()
    gap_m, gap_i = _maxerr(masks, ref_masks), _maxerr(iou, ref_iou)
    print(f"\n[cfg2 vs reference cdist mode] groups with identical kNN set {knn_same:.4f}, points with identical 3-NN set {nn3_same:.5f}, "
          f"logit gap {gap_m:.2e}, iou gap {gap_i:.2e}")
    assert knn_same > 0.98 and nn3_same > 0.995
    assert gap_m < TOL and gap_i < TOL, (gap_m, gap_i)


def test_against_reference_demo_plys(gpu, golden_ply):
    """The reference's only real inputs (demo/static/models/*.ply; up to 7276 exact duplicate points) run through the reference's
    own modules (tests/golden/make_golden.py::make_ply_cases): FPS indices bit-identical on all six, neighbour sets equal up to
    exact ties (duplicate points), encoder embeddings and logits within tolerance."""
    from conftest import ply_cases
    meta, _ = golden_ply
    cfg = get_config(meta["cfg"], meta["G"], meta["K"])
    sd = random_state_dict(cfg, seed=meta["seed"])
    assert state_dict_checksum(sd) == pytest.approx(meta["weights_checksum"], rel=1e-12)
    model = gpu(cfg, sd, precision="f16x3")
    for key, xyz, rgb, a in ply_cases(golden_ply):
        st = model.encode(xyz.cuda(), rgb.cuda())
        assert torch.equal(st.fps_idx.cpu()[0].to(torch.int32), a["fps_idx"]), f"{key}: FPS indices differ"
        got, want = st.knn_idx.cpu()[0].sort(-1).values, a["knn_idx"].long().sort(-1).values
        diff = (got != want).any(-1)
        if bool(diff.any()):   # neighbour sets may differ only by points at EXACTLY the same distance (duplicates) or within cdist's rounding
            c = st.centers.cpu()[0].double()
            def d2(idx):
                return ((xyz[0].double()[idx] - c[:, None, :]) ** 2).sum(-1).sort(-1).values
            assert (d2(got)[diff] - d2(want)[diff]).abs().max() < 1e-6, f"{key}: kNN sets differ beyond ties"
        prompt = xyz[0][a["prompt_idx"][0].long()][None].cuda()
        masks, iou = model.decode(st, prompt, torch.ones(1, 1, dtype=torch.int64, device="cuda"), None, True)
        e_emb, e_m, e_i = _maxerr(st.pc_embeddings[0], a["pc_embeddings"]), _maxerr(masks[0], a["masks"]), _maxerr(iou[0], a["iou"])
        print(f"\n[{key}] N={xyz.shape[1]} groups with a different (tied) neighbour set {int(diff.sum())}/{len(diff)}; max|err| emb {e_emb:.2e} masks {e_m:.2e} iou {e_i:.2e}")
        assert e_m < TOL and e_i < TOL and e_emb < TOL, key
    model.check_coordinate_range()


def test_forward_eval_protocol(gpu, golden_forward):
    """model(coords, features, gt_masks, is_eval=True) -- the reference's evaluation entry point (eval_kitti.py:363) --
    against the golden run of the reference's own PointCloudSAM.forward and against the oracle."""
    meta, a = golden_forward
    cfg = get_config(meta["cfg"])
    sd = random_state_dict(cfg, seed=meta["seed"])
    for precision in ("f32", "bf16x6", "f16x3"):
        model = gpu(cfg, sd, precision=precision)
        model.prompt_iters = meta["iters"]
        outs = model(a["xyz"].cuda(), a["rgb"].cuda(), a["gt_masks"].cuda(), is_eval=True)
        assert len(outs) == meta["iters"]
        for i, o in enumerate(outs):
            assert torch.equal(o["prompt_coords"].cpu(), a[f"prompt_coords_{i}"]), f"iteration {i}: simulated click differs from the reference"
            assert torch.equal(o["prompt_labels"].cpu(), a[f"prompt_labels_{i}"])
            assert _maxerr(o["masks"], a[f"masks_{i}"]) < TOL and _maxerr(o["iou_preds"], a[f"iou_preds_{i}"]) < TOL
            assert _maxerr(o["prompt_masks"], a[f"prompt_masks_{i}"]) < TOL
    # sampler branches (false positives only / no error at all) against the oracle
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(2, 700, 3, generator=g) * 2 - 1
    gt = torch.stack([pts[..., 0] > 0, pts[..., 1] > 0.3], 1)
    for logits in (torch.full((4, 700), 5.0), torch.where(gt.reshape(4, 700), 5.0, -5.0), torch.randn(4, 700, generator=g)):
        wc, wl = O.sample_eval_prompts(pts, gt, logits)
        gc, gl = model.sample_prompts(pts.cuda(), gt.cuda(), logits.cuda(), is_eval=True)
        assert torch.equal(gc.cpu(), wc) and torch.equal(gl.cpu(), wl)


def test_evaluation_harness(gpu):
    """IoU@click loop of evaluation/eval_kitti.py on synthetic labelled clouds: runs, shapes, and IoU values equal to the
    oracle's protocol on the same data."""
    import numpy as np
    from point_sam_amd import evaluation as E
    cfg = get_config("tiny", 48, 24)
    sd = random_state_dict(cfg, 6)
    model = gpu(cfg, sd)
    model.prompt_iters = 3
    rng = np.random.default_rng(1)
    samples, want = [], []
    for n in (900, 1300):
        xyz = rng.normal(size=(n, 3)) * [2.0, 1.0, 0.5] + 4
        rgb = rng.integers(0, 256, size=(n, 3)).astype(np.float64)
        labels = (xyz[:, 0] > 4).astype(np.int64) + 2 * (xyz[:, 1] > 4.3)     # 4 instances
        d = E.prepare_sample(xyz, rgb, labels)
        samples.append(d)
        outs = O.forward_eval(sd, cfg, d["coords"].cpu(), d["features"].cpu(), d["gt_masks"].cpu(), prompt_iters=3)
        gtf = d["gt_masks"].cpu().flatten(0, 1)
        want.append([E.compute_iou(o["prompt_masks"], gtf).mean().item() for o in outs])
    res = E.evaluate_clouds(model, samples, adapt_grouper=False)
    assert res["per_cloud"].shape == (2, 3)
    assert np.allclose(res["per_cloud"], np.array(want), atol=2e-3), (res["per_cloud"], want)


def test_graph_pipeline_with_in_kernel_fixups_matches_eager(gpu):
    """Graphs whose kernels carry per-stream fix-up state -- the split-K GEMMs and the key-split attention of a single cloud through the giant
    encoder's width (arrival counters per (device, stream), csrc/gemm_f16x3p.hip / attention.hip) -- replayed with more slots than dense streams: every
    step's result must be the eager path's bits.  (Until round 5 a slot's graph could replay on another stream than it was captured on; two graphs
    holding the same counters then ran concurrently and a tile could be combined before all of its parts had arrived.)"""
    from point_sam_amd.model import GraphPipeline
    cfg = _giant_slim()
    model = gpu(cfg, random_state_dict(cfg, 14), precision="f16x3")
    batches = []
    for i in range(14):
        xyz, rgb, prompt, labels = O.synthetic_batch(1, 4096, seed=60 + i)
        batches.append(tuple(t.cuda() for t in (xyz, rgb, prompt, labels)))
    from point_sam_amd import ops
    with ops.attention_keysplit(1):      # what the multi-stream pipelines run with
        want = [model.predict_masks(*b) for b in batches]
    pipe = GraphPipeline(model, *batches[0], None, True, slots=3, dense_streams=2)
    assert pipe.depth % len(pipe.dense) == 0 and all(st.ds is pipe.dense[k % len(pipe.dense)] for k, st in enumerate(pipe.slots))
    got = []
    for k in range(min(pipe.depth, len(batches))):
        pipe.submit(*batches[k])
    for k in range(len(batches)):
        m, i = pipe.next()
        got.append((m.clone(), i.clone()))
        if k + pipe.depth < len(batches):
            pipe.submit(*batches[k + pipe.depth])
    torch.cuda.synchronize()
    for k, ((m1, i1), (m2, i2)) in enumerate(zip(want, got)):
        assert torch.equal(m1, m2) and torch.equal(i1, i2), (k, _maxerr(m1, m2))


def test_captured_graph_replays_on_another_stream_beside_eager_launches(gpu):
    """the in-kernel fix-ups (split-K GEMMs, key-split attention, fused Linear + LayerNorm of the decoder) count in through an
    arrival-counter block the CALLER owns (ops.new_counters / use_counters); the library keeps no (device, stream) state.  So a graph captured with a block
    of its own replays bit-identically on ANOTHER stream, while the capture stream runs eager launches of the same kernels (which use that stream's
    block).  Giant width, one cloud: every fix-up kernel is on the path."""
    from point_sam_amd import ops
    cfg = _giant_slim()
    model = gpu(cfg, random_state_dict(cfg, 14), precision="f16x3")
    xyz, rgb, prompt, labels = (t.cuda() for t in O.synthetic_batch(1, 4096, seed=71))
    xyz2, rgb2, prompt2, labels2 = (t.cuda() for t in O.synthetic_batch(1, 4096, seed=72))
    want = model.predict_masks(xyz, rgb, prompt, labels)
    want2 = model.predict_masks(xyz2, rgb2, prompt2, labels2)
    cap, other = torch.cuda.Stream(), torch.cuda.Stream()
    block = ops.new_counters(xyz.device)
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap), ops.use_counters(block):
        model.predict_masks(xyz, rgb, prompt, labels)
    cap.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap), ops.use_counters(block):
        out = model.predict_masks(xyz, rgb, prompt, labels, validate=False)
    torch.cuda.synchronize()
    for _ in range(4):
        with torch.cuda.stream(other):
            g.replay()
        with torch.cuda.stream(cap):      # eager launches of the same kernels on the capture stream, concurrently
            got2 = model.predict_masks(xyz2, rgb2, prompt2, labels2)
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]), "graph replayed on another stream: other bits"
        assert torch.equal(got2[0], want2[0]) and torch.equal(got2[1], want2[1]), "eager launches beside the replay: other bits"
        assert int(block.abs().max()) == 0, "a launch left its arrival counters non-zero"


def test_graph_pipeline_matches_eager(gpu):
    """The two stages of a batch replayed as captured HIP graphs (GraphPipeline: static buffers, `slots` batches in flight) give
    bit-identical results to the eager path, also when the inputs change from step to step."""
    from point_sam_amd.model import GraphPipeline
    cfg = get_config("tiny", 64, 16)
    model = gpu(cfg, random_state_dict(cfg, 4), precision="f16x3")
    batches = []
    for i in range(7):
        xyz, rgb, prompt, labels = O.synthetic_batch(2, 3000, seed=40 + i)
        batches.append(tuple(t.cuda() for t in (xyz, rgb, prompt, labels)))
    want = [model.predict_masks(*b) for b in batches]
    pipe = GraphPipeline(model, *batches[0], None, True, slots=3, dense_streams=2)
    got = []
    for k in range(min(pipe.depth, len(batches))):
        pipe.submit(*batches[k])
    with pytest.raises(RuntimeError):
        pipe.submit(*batches[0])                     # all slots in flight
    for k in range(len(batches)):
        m, i = pipe.next()
        got.append((m.clone(), i.clone()))           # static outputs: copy before the slot is reused
        if k + pipe.depth < len(batches):
            pipe.submit(*batches[k + pipe.depth])
    torch.cuda.synchronize()
    for (m1, i1), (m2, i2) in zip(want, got):
        assert torch.equal(m1, m2) and torch.equal(i1, i2)
    model.check_coordinate_range()
    # a replay computes on the captured buffers only: anything the graphs were not captured for is refused, not silently ignored
    xyz, rgb, prompt, labels = batches[0]
    with pytest.raises(ValueError):
        pipe.submit(xyz[:1], rgb[:1], prompt[:1], labels[:1])                                  # smaller batch (copy_ would broadcast it)
    with pytest.raises(ValueError):
        pipe.submit(xyz, rgb, prompt, labels, torch.zeros(2, 3000, device="cuda"))            # captured without a mask prompt
    g = model.pc_encoder.patch_embed.grouper
    g.num_groups = 32
    with pytest.raises(ValueError):
        pipe.submit(xyz, rgb, prompt, labels)                                                  # grouper changed after capture
    g.num_groups = 64
    pipe.submit(xyz, rgb, prompt, labels)
    m, i = pipe.next()
    assert torch.equal(m, want[0][0]) and torch.equal(i, want[0][1])


def test_pipelines_bitwise_equal_eager_at_bench_config(gpu):
    """The benchmark's own configuration (BASELINE configs[1]: ViT-L, B=8, N=32768, 512x64; two dense streams + the tokenizer stream; HIP
    graphs, 3 slots) gives, step after step, the bits of the plain single-stream predict_masks.  (The small-config graph test above did not
    see round 3's epilogue race: it needs full-size GEMMs of two batches sharing the CUs.)"""
    from point_sam_amd.model import BatchPipeline, GraphPipeline
    cfg = get_config("large", 512, 64)
    model = gpu(cfg, random_state_dict(cfg, 42), precision="f16x3")
    batch = tuple(t.cuda() for t in O.synthetic_batch(8, 32768, seed=42))
    want_m, want_i = model.predict_masks(*batch)
    torch.cuda.synchronize()

    def run(pipe, n=6):
        for k in range(min(pipe.depth, n)):
            pipe.submit(*batch, None, True)
        for k in range(n):
            m, i = pipe.next()
            assert torch.equal(m, want_m) and torch.equal(i, want_i), (type(pipe).__name__, k, float((m - want_m).abs().max()))
            if k + pipe.depth < n:
                pipe.submit(*batch, None, True)
        torch.cuda.synchronize()

    run(BatchPipeline(model, dense_streams=2))
    run(GraphPipeline(model, *batch, None, True, slots=3, dense_streams=2))
    model.check_coordinate_range()


def _nccl_worker(rank, world, port, q):
    import os, sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from point_sam_amd import dist as psdist
    from point_sam_amd.model import PointCloudSAM
    r, w, local = psdist.init_from_env(backend="nccl")
    torch.cuda.set_device(local)
    cfg = get_config("tiny", 64, 16)
    sd = random_state_dict(cfg, 5)
    total = 4
    xyz, rgb, prompt, labels = O.synthetic_batch(total, 4000, seed=9)
    lo, hi = psdist.shard_range(total, r, w)
    model = PointCloudSAM(cfg, sd, f"cuda:{local}", precision="f16x3")
    dev = lambda t: t[lo:hi].contiguous().to(f"cuda:{local}")
    masks, iou = model.predict_masks(dev(xyz), dev(rgb), dev(prompt), dev(labels))
    g = psdist.SideStreamGather(torch.device("cuda", local))
    all_masks, all_iou = g.finish(g.start((masks, iou), total))
    torch.cuda.synchronize()
    if r == 0:
        # the same shards run one after the other on this rank: bit-identical (same kernels on the same shapes); the whole batch at once
        # picks other GEMM tiles for its other row counts: equal within rounding
        full = lambda t: t.to(f"cuda:{local}")
        parts = []
        for rr in range(w):
            l2, h2 = psdist.shard_range(total, rr, w)
            cut = lambda t: t[l2:h2].contiguous().to(f"cuda:{local}")
            parts.append(model.predict_masks(cut(xyz), cut(rgb), cut(prompt), cut(labels)))
        seq_masks, seq_iou = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        ref_masks, ref_iou = model.predict_masks(full(xyz), full(rgb), full(prompt), full(labels))
        close = float((all_masks - ref_masks).abs().max()) < 1e-4 and float((all_iou - ref_iou).abs().max()) < 1e-4
        q.put((bool(torch.equal(all_masks, seq_masks)) and close, bool(torch.equal(all_iou, seq_iou)), tuple(all_masks.shape)))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_over_rccl_match_one_rank(gpu):
    """BASELINE config #4's mechanism on two GPUs of one node (skipped with fewer): one process per GPU, each rank runs its shard of
    the clouds, the logits are all-gathered over RCCL on a side stream; the gathered result equals the same shards run on one rank bit
    for bit, and the whole batch run at once within rounding (clouds never interact; other row counts pick other GEMM tiles)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_nccl_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    ok_m, ok_i, shape = q.get(timeout=10)
    assert ok_m and ok_i and shape[0] == 4


def test_click_session_eager_graph_and_oracle(gpu):
    """The interactive session (BASELINE config #5's flow: encoder once, T decodes, each with all clicks so far and the previous best mask;
    pc_sam.py:139-194): PointCloudSAM.click_session equals the predictor-style loop bit for bit, the captured form
    (GraphPipeline(session=True)) equals the eager one, and the last click matches the oracle's click loop."""
    from point_sam_amd.model import GraphPipeline
    cfg = get_config("tiny", 64, 16)
    sd = random_state_dict(cfg, 6)
    model = gpu(cfg, sd, precision="f16x3")
    B, N, T = 2, 2500, 4
    xyz, rgb, _, _ = O.synthetic_batch(B, N, seed=70)
    g = torch.Generator().manual_seed(2)
    clicks = torch.stack([xyz[b, torch.randint(0, N, (T,), generator=g)] for b in range(B)])
    labels = torch.tensor([[1, 1, 0, 1]]).repeat(B, 1)
    xd, rd, cd, ld = xyz.cuda(), rgb.cuda(), clicks.cuda(), labels.cuda()
    st = model.encode(xd, rd)
    outs = model.click_session(st, cd, ld)
    # the same loop written out
    best, ref = None, []
    for t in range(T):
        m, i = model.decode(st, cd[:, : t + 1].contiguous(), ld[:, : t + 1].contiguous(), best, best is None)
        ref.append((m, i))
        best = torch.gather(m, 1, i.argmax(1).view(-1, 1, 1).expand(-1, 1, N))[:, 0] if t == 0 else m[:, 0]
    for (m1, i1), (m2, i2) in zip(outs, ref):
        assert torch.equal(m1, m2) and torch.equal(i1, i2)
    pipe = GraphPipeline(model, xd, rd, cd, ld, None, True, slots=2, dense_streams=2, session=True)
    for _ in range(2):
        pipe.submit(xd, rd, cd, ld)
    for _ in range(2):
        m, i = pipe.next()
        assert torch.equal(m, outs[-1][0]) and torch.equal(i, outs[-1][1])
    want = [O.click_loop(sd, cfg, xyz[b:b + 1], rgb[b:b + 1], clicks[b:b + 1], labels[b:b + 1])[-1] for b in range(B)]
    for b in range(B):
        assert _maxerr(outs[-1][0][b:b + 1], want[b][0]) < TOL and _maxerr(outs[-1][1][b:b + 1], want[b][1]) < TOL
    model.check_coordinate_range()
