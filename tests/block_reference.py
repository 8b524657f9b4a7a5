"""fp64 references of the five coarse entries of csrc/blocks.hip, one per entry, built from oracle/pointsam_oracle.py (dtype-generic) on a state dict
cast to double; the same functions in fp32 give the yardstick e32 of tests/test_blocks_cpu.py and tests/test_gpu_blocks.py.  Weights come from a
seeded generator under the names the _Stage classes of point_sam_amd/ops.py bind; heavy_tailed() turns them into the trained-checkpoint-like statistics
the a-priori bounds of the packed hand-overs (qkv_bound, v_bound, u_c0..2, k1 / k2, ln21_bound) have to survive.  problem(case) -> (state dict, inputs,
fp64 outputs, e32 per output) is computed once per case and shared by both test files."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import block_cases as BC
from oracle import pointsam_oracle as O
from point_sam_amd.config import ViTConfig

EVA_EPS, LN_EPS = 1e-6, 1e-5
BLK, PATCH, TW = "blk", "enc", "mask_decoder.transformer"


# ------------------------------------------------------------------------------------------------ weights
def _fill(shapes, seed):
    """Linear weights N(0, 1 / fan_in), biases 0.02 N, LayerNorm gains 1 + 0.1 N and offsets 0.1 N (as point_sam_amd.weights.random_state_dict)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in shapes:
        if "norm" in name or name.endswith((".conv1.1.weight", ".conv1.1.bias", ".conv2.1.weight", ".conv2.1.bias", "upscaling.1.weight", "upscaling.1.bias")):
            t = torch.randn(shape, generator=g) * 0.1 + (1.0 if name.endswith("weight") else 0.0)
        elif len(shape) == 2:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        else:
            t = torch.randn(shape, generator=g) * 0.02
        sd[name] = t.contiguous()
    return sd


def _linear(name, fout, fin, bias=True):
    return [(name + ".weight", (fout, fin))] + ([(name + ".bias", (fout,))] if bias else [])


def _norm(name, n):
    return [(name + ".weight", (n,)), (name + ".bias", (n,))]


def eva_weights(dim, hidden, seed):
    p = BLK
    return _fill(_norm(p + ".norm1", dim) + _linear(p + ".attn.q_proj", dim, dim) + _linear(p + ".attn.k_proj", dim, dim, False) + _linear(p + ".attn.v_proj", dim, dim)
                 + _linear(p + ".attn.proj", dim, dim) + _norm(p + ".norm2", dim) + _linear(p + ".mlp.fc1_g", hidden, dim) + _linear(p + ".mlp.fc1_x", hidden, dim)
                 + _norm(p + ".mlp.norm", hidden) + _linear(p + ".mlp.fc2", dim, hidden), seed)


def gelu_weights(dim, hidden, seed):
    p = BLK
    return _fill(_norm(p + ".norm1", dim) + [(p + ".attn.qkv.weight", (3 * dim, dim)), (p + ".attn.q_bias", (dim,)), (p + ".attn.v_bias", (dim,))]
                 + _linear(p + ".attn.proj", dim, dim) + _norm(p + ".norm2", dim) + _linear(p + ".mlp.fc1", hidden, dim) + _linear(p + ".mlp.fc2", dim, hidden), seed)


def patch_weights(cin, h0, h1, cout, seed):
    p = PATCH
    return _fill(_linear(p + ".conv1.0", h0, cin) + _norm(p + ".conv1.1", h0) + _linear(p + ".conv1.3", h0, h0) + _linear(p + ".conv2.0", h1, 2 * h0) + _norm(p + ".conv2.1", h1)
                 + _linear(p + ".conv2.3", cout, h1), seed)


def upscale_weights(dim, seed):
    p = "mask_decoder.output_upscaling"
    return _fill(_linear(p + ".0", dim, dim) + _norm(p + ".1", dim) + _linear(p + ".3", dim, dim), seed)


def twoway_weights(depth, E, mlp, downsample, seed):
    IX = E // downsample

    def attn(p, inner):
        return _linear(p + ".q_proj", inner, E) + _linear(p + ".k_proj", inner, E) + _linear(p + ".v_proj", inner, E) + _linear(p + ".out_proj", E, inner)
    shapes = []
    for i in range(depth):
        L = f"{TW}.layers.{i}"
        shapes += attn(L + ".self_attn", E) + _norm(L + ".norm1", E) + attn(L + ".cross_attn_token_to_image", IX) + _norm(L + ".norm2", E)
        shapes += _linear(L + ".mlp.lin1", mlp, E) + _linear(L + ".mlp.lin2", E, mlp) + _norm(L + ".norm3", E) + _norm(L + ".norm4", E) + attn(L + ".cross_attn_image_to_token", IX)
    shapes += attn(TW + ".final_attn_token_to_image", IX) + _norm(TW + ".norm_final_attn", E)
    return _fill(shapes, seed)


def heavy_tailed(sd, seed, gain=15.0):
    """Trained-checkpoint-like statistics on top of the seeded Gaussians, made the way tests/test_gpu_e2e.py::_heavy_tailed makes them: 1 % of the LayerNorm
    gains `gain` x and offsets of a few units, sparse 30 x weights, 1 % loud output rows, 1 % of the input columns 8 x, bias outliers.  The stages here
    are small, so at least one gain, one output row, one column and one bias of every tensor are hot."""
    g = torch.Generator().manual_seed(seed)
    out = {}

    def some(shape, p):      # a mask with probability p and at least one hit
        m = torch.rand(shape, generator=g) < p
        m.view(-1)[int(torch.randint(m.numel(), (1,), generator=g))] = True
        return m
    for k, v in sd.items():
        t = v.clone()
        norm = "norm" in k or ".conv1.1." in k or ".conv2.1." in k or "upscaling.1." in k
        if norm and t.dim() == 1:
            hot = some(t.shape, 0.01)
            t = torch.where(hot, t * gain if k.endswith("weight") else t + 3.0 * torch.sign(torch.randn(t.shape, generator=g)), t)
        elif t.dim() == 2 and min(t.shape) >= 64:
            t = torch.where(torch.rand(t.shape, generator=g) < 5e-4, t * 30.0, t)
            t = t * torch.where(some((t.shape[0], 1), 0.01), gain, 1.0)
            t = t * torch.where(some((1, t.shape[1]), 0.01), 8.0, 1.0)
        elif t.dim() == 1:
            t = torch.where(some(t.shape, 0.01), t + 2.0 * torch.sign(torch.randn(t.shape, generator=g)), t)
        out[k] = t.contiguous()
    return out


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ the references (dtype: torch.float64 / torch.float32)
def eva_reference(sd, x, dim, heads, hidden, swiglu, dtype):
    """x [B, L, dim] -> [B * L, dim]: oracle eva_block with a ViTConfig of the case's dims."""
    vit = ViTConfig("case", dim, 1, heads, hidden, swiglu, EVA_EPS)
    return O.eva_block(cast(sd, dtype), BLK, x.to(dtype), vit).reshape(-1, dim)


def patch_reference(sd, xyz, feats, centers, knn_idx, center_idx, radius, dtype):
    """xyz [B, N, 3], feats [B * rep, N, C], centers [B, G, 3], knn_idx [B, G, K], center_idx [B, G] or None -> [B * rep * G, cout]."""
    rep = feats.shape[0] // xyz.shape[0]
    r = lambda t: None if t is None else t.repeat_interleave(rep, 0)
    patches = O.group_points(r(xyz).to(dtype), feats.to(dtype), r(centers).to(dtype), r(knn_idx), radius or None, r(center_idx))
    out = O.patch_encoder(cast(sd, dtype), PATCH, patches, LN_EPS)
    return out.reshape(-1, out.shape[-1])


def upscale_reference(sd, keys, idx3, w3, hyper, rep, dtype):
    """keys [Z, G, E], idx3 / w3 [Z / rep, N, 3], hyper [Z, C, E] -> masks [Z, C, N]."""
    w, p = cast(sd, dtype), "mask_decoder.output_upscaling"
    up = O.interpolate(keys.to(dtype), idx3.repeat_interleave(rep, 0), w3.to(dtype).repeat_interleave(rep, 0))
    up = F.gelu(O._ln(w, p + ".1", O._lin(w, p + ".0", up), LN_EPS))
    up = F.gelu(O._lin(w, p + ".3", up))
    return hyper.to(dtype) @ up.transpose(1, 2)


def twoway_reference(sd, depth, heads, keys, pos, tokens, rep, dtype):
    """keys [Z, G, E], pos [Z / rep, G, E], tokens [Z, T, E] -> (queries [Z * T, E], keys [Z * G, E])."""
    ns = SimpleNamespace(dec_depth=depth, dec_heads=heads, ln_eps=LN_EPS)
    q, k = O.two_way_transformer(cast(sd, dtype), ns, keys.to(dtype), pos.to(dtype).repeat_interleave(rep, 0), tokens.to(dtype))
    E = q.shape[-1]
    return q.reshape(-1, E), k.reshape(-1, E)


def rel_err(y, y64):
    """max |y - y64| / max(1, max |y64|)"""
    y64 = y64.detach().cpu().double()
    return ((y.detach().cpu().double() - y64).abs().max() / max(1.0, y64.abs().max().item())).item()


# ------------------------------------------------------------------------------------------------ weights, inputs and references of a case
def case_weights(c):
    if isinstance(c, BC.EvaCase):
        sd = eva_weights(c.dim, c.hidden, c.seed)
    elif isinstance(c, BC.GeluCase):
        sd = gelu_weights(c.dim, c.hidden, c.seed)
    elif isinstance(c, BC.PatchCase):
        sd = patch_weights(BC.patch_cin(c), 128, c.h1, c.cout, c.seed)
    elif isinstance(c, BC.UpscaleCase):
        sd = upscale_weights(c.dim, c.seed)
    else:
        sd = twoway_weights(c.depth, c.E, c.mlp, c.downsample, c.seed)
    return heavy_tailed(sd, c.seed + 1) if getattr(c, "heavy", False) else sd


def case_inputs(c):
    """The case's input tensors (CPU, fp32), seeded."""
    g = torch.Generator().manual_seed(c.seed + 7)
    rn = lambda *s: torch.randn(*s, generator=g)
    if isinstance(c, (BC.EvaCase, BC.GeluCase)):
        return dict(x=rn(c.B, c.L, c.dim))
    if isinstance(c, BC.PatchCase):
        C = c.C
        xyz = torch.rand(c.B, c.N, 3, generator=g) * 2 - 1
        knn_idx = torch.randint(c.N, (c.B, c.G, c.K), generator=g)
        center_idx = torch.randint(c.N, (c.B, c.G), generator=g)
        knn_idx[:, :, 0] = center_idx      # a group holds its centre
        centers = torch.gather(xyz, 1, center_idx.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        return dict(xyz=xyz, feats=torch.rand(c.B * c.rep, c.N, C, generator=g), centers=centers, knn_idx=knn_idx, center_idx=center_idx if c.centralize else None)
    if isinstance(c, BC.UpscaleCase):
        B = max(c.Z // c.rep, 1)
        return dict(keys=rn(c.Z, c.G, c.dim), hyper=rn(c.Z, c.C, c.dim), xyz=torch.rand(B, c.N, 3, generator=g) * 2 - 1, centers=torch.rand(B, c.G, 3, generator=g) * 2 - 1)
    return dict(tokens=rn(c.Z, c.T, c.E), keys=rn(c.Z, c.G, c.E), pos=rn(max(c.Z // c.rep, 1), c.G, c.E))


def three_nn_cpu(xyz, centers, eps=1e-8):
    """compute_interp_weights in plain torch (fp32): the CPU stand-in of ops.three_nn for the reference-health check; the GPU test uses ops.three_nn."""
    d2 = ((xyz.unsqueeze(2) - centers.unsqueeze(1)) ** 2).sum(-1)
    d, idx = torch.topk(d2, 3, dim=2, largest=False)
    inv = 1.0 / torch.clamp(d, min=eps)
    return idx, (inv / inv.sum(2, keepdim=True)).contiguous()


def reference(c, sd, inp, dtype):
    """-> list of output tensors.  An UpscaleCase needs inp['idx3'] / inp['w3']."""
    if isinstance(c, BC.EvaCase):
        return [eva_reference(sd, inp["x"], c.dim, c.dim // 64, c.hidden, True, dtype)]
    if isinstance(c, BC.GeluCase):
        return [eva_reference(sd, inp["x"], c.dim, c.heads, c.hidden, False, dtype)]
    if isinstance(c, BC.PatchCase):
        return [patch_reference(sd, inp["xyz"], inp["feats"], inp["centers"], inp["knn_idx"], inp["center_idx"], c.radius, dtype)]
    if isinstance(c, BC.UpscaleCase):
        return [upscale_reference(sd, inp["keys"], inp["idx3"], inp["w3"], inp["hyper"], c.rep, dtype)]
    return list(twoway_reference(sd, c.depth, c.heads, inp["keys"], inp["pos"], inp["tokens"], c.rep, dtype))


def _key(c):      # cases that differ in launch sequence, key split or counters only share their problem
    drop = {"keysplit", "counters", "mode", "edge", "want", "refused"}
    return (type(c).__name__,) + tuple(v for f, v in zip(c._fields, c) if f not in drop)


_PROBLEMS = {}


def problem(c, idx3=None, w3=None):
    """(state dict, inputs, fp64 outputs, e32 per output) of a case, computed once.  idx3 / w3: the 3-NN plan of an UpscaleCase (default: three_nn_cpu)."""
    k = _key(c) + (idx3 is not None,)
    if k not in _PROBLEMS:
        sd, inp = case_weights(c), case_inputs(c)
        if isinstance(c, BC.UpscaleCase):
            inp["idx3"], inp["w3"] = three_nn_cpu(inp["xyz"], inp["centers"]) if idx3 is None else (idx3, w3)
        with torch.no_grad():
            y64 = reference(c, sd, inp, torch.float64)
            e32 = [rel_err(a, b) for a, b in zip(reference(c, sd, inp, torch.float32), y64)]
        _PROBLEMS[k] = (sd, inp, y64, e32)
    return _PROBLEMS[k]
