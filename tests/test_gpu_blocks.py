"""The five coarse C-ABI entries of csrc/blocks.hip -- psam_eva_block, psam_eva_gelu_block, psam_patch_encoder, psam_upscale_masks, psam_twoway_decoder --
each ALONE (one stage prepared through ops.EvaBlock / EvaGeluBlock / CPatchEncoder / CUpscale / CTwoWay from a dict of device tensors, no PointCloudSAM),
at the cases of tests/block_cases.py: the smallest shapes at which every shape-dependent branch of the host sequencing exists
(tests/test_blocks_cpu.py keeps the lists equal to the thresholds in the sources).  Every case
  1. is compared with the fp64 oracle of tests/block_reference.py: e = max |y - y64| / max(1, max |y64|) per output must satisfy
     e_gpu <= C_BOUND * e32 + 1e-7, e32 the error of the SAME oracle in fp32 on the same inputs (the figures are printed: `[ratio] ...`);
  2. gives the same bits twice;
  3. runs on a workspace of exactly *_ws_bytes between two guards (workspace_check.check_exact_workspace): guards intact, the bits of the call on a
     workspace of its own, PSAM_EWORKSPACE with one byte less and nothing touched;
  4. leaves the sentinel rows behind its in-place / caller-provided outputs alone.
A case the entry must refuse answers PSAM_EINVAL with psam_last_error_string() naming the entry, before anything is launched: every output buffer and a
0xA5-filled workspace (or prepared blob) keep their bits."""
import ctypes

import pytest
import torch

import block_cases as BC
import block_reference as BR
from workspace_check import check_exact_workspace

pytestmark = pytest.mark.gpu

# The project's own GEMM class (errs["f16x3"] < 4 * errs["f32"], tests/test_gpu_kernels.py) times two for the packed hand-overs, which round once more
# than an fp32 chain.  Measured ratios: profiles/blocks/ratios.md.
C_BOUND = 8.0
SENT = -54321.0
PAD = 8              # sentinel rows behind every output
EINVAL = -1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from point_sam_amd import ops as _ops
    _ops._lib.load()
    return _ops


@pytest.fixture(scope="module")
def stages(ops):
    """Every weight set is prepared once: weights key -> (stage, device state dict)."""
    cache = {}

    def get(c):
        k = ("w",) + tuple(v for f, v in zip(c._fields, c) if f in WEIGHT_FIELDS[type(c)])
        if k not in cache:
            sd = {n: t.cuda().contiguous() for n, t in BR.case_weights(c).items()}
            cache[k] = (build_stage(ops, c, sd), sd)
            torch.cuda.synchronize()
        return cache[k][0]
    return get


WEIGHT_FIELDS = {BC.EvaCase: ("dim", "hidden", "heavy", "seed"), BC.GeluCase: ("dim", "heads", "hidden", "seed"), BC.PatchCase: ("h1", "cout", "C", "centralize", "cin", "heavy", "seed"),
                 BC.UpscaleCase: ("dim", "heavy", "seed"), BC.TwowayCase: ("depth", "E", "heads", "mlp", "downsample", "heavy", "seed")}


def build_stage(ops, c, sd, cls=None):
    if isinstance(c, BC.EvaCase):
        return (cls or ops.EvaBlock)(sd, BR.BLK, c.dim, c.dim // 64, c.hidden, BR.EVA_EPS)
    if isinstance(c, BC.GeluCase):
        return (cls or ops.EvaGeluBlock)(sd, BR.BLK, c.dim, c.heads, c.hidden, BR.EVA_EPS)
    if isinstance(c, BC.PatchCase):
        return (cls or ops.CPatchEncoder)(sd, BR.PATCH, BR.LN_EPS)
    if isinstance(c, BC.UpscaleCase):
        return (cls or ops.CUpscale)(sd, BR.LN_EPS)
    return (cls or ops.CTwoWay)(sd, BR.TW, c.depth, c.E, c.heads, c.mlp, c.downsample, BR.LN_EPS)


def raw_prepare(ops, base, *args):
    """The stage's weight struct as `base` fills it, handed to ENTRY_prepare on a 0xA5-filled blob -> (status, message, blob untouched)."""
    got = {}

    class Probe(base):
        def _prepare(self, wt, plan, *dims):
            got.update(wt=wt, plan=plan, dims=dims)
    keep = Probe(*args)
    lib = ops._lib.load()
    need = int(getattr(lib, base.ENTRY + "_prepared_bytes")(*got["dims"]))
    blob = torch.full((max(need, 4096),), 0xA5, dtype=torch.uint8, device="cuda")
    status = getattr(lib, base.ENTRY + "_prepare")(ctypes.byref(got["wt"]), ctypes.byref(got["plan"]), blob.data_ptr(), blob.numel(), ops._stream())
    msg = lib.psam_last_error_string().decode()
    torch.cuda.synchronize()
    del keep
    return status, msg, bool((blob == 0xA5).all())


def padded(rows, cols):
    """[rows, cols] view of a buffer with PAD sentinel rows behind it -> (buffer, view)."""
    buf = torch.full((rows + PAD, cols), SENT, device="cuda")
    return buf, buf[:rows]


class Runner:
    """One case on the GPU: call(ws, ws_bytes) -> status through the C ABI, reset() puts back what the call updates or writes, outputs() are those tensors,
    bufs the sentinel-padded buffers behind them."""

    def __init__(self, ops, c, stage, inp):
        lib = self.lib = ops._lib.load()
        self.c, self.bufs, self.entry = c, [], stage.ENTRY
        cu = lambda t: None if t is None else t.cuda().contiguous()
        s = ops._stream
        if isinstance(c, (BC.EvaCase, BC.GeluCase)):
            M = c.B * c.L
            x0 = cu(inp["x"].reshape(M, c.dim))
            buf, x = padded(M, c.dim)
            self.bufs, self.outs, self.reset = [(buf, M)], [x], lambda: x.copy_(x0)
            self.need = int(getattr(lib, self.entry + "_ws_bytes")(M, c.dim, c.hidden))
            if isinstance(c, BC.EvaCase):
                self.call = lambda ws, n: lib.psam_eva_block(ctypes.byref(stage.plan), stage.blob.data_ptr(), x.data_ptr(), c.B, c.L, ws, n, s())
            else:
                plan = ops._lib.EvaGeluBlockPlan.from_buffer_copy(stage.plan)
                plan.attn_keysplit = c.keysplit
                cnt = ops.arrival_counters(x.device).data_ptr() if c.counters else None
                self.call = lambda ws, n: lib.psam_eva_gelu_block(ctypes.byref(plan), stage.blob.data_ptr(), x.data_ptr(), c.B, c.L, ws, n, cnt, s())
        elif isinstance(c, BC.PatchCase):
            groups = c.B * c.rep * c.G
            xyz, feats, centers, knn, cidx = cu(inp["xyz"]), cu(inp["feats"]), cu(inp["centers"]), cu(inp["knn_idx"]), cu(inp["center_idx"])
            buf, out = padded(groups, c.cout)
            self.keep = (xyz, feats, centers, knn, cidx)
            self.bufs, self.outs, self.reset = [(buf, groups)], [out], lambda: out.fill_(-7.0)
            self.need = int(lib.psam_patch_encoder_ws_bytes(groups * c.K, groups, stage.h0, stage.h1))
            self.call = lambda ws, n: lib.psam_patch_encoder(ctypes.byref(stage.plan), stage.blob.data_ptr(), xyz.data_ptr(), feats.data_ptr(), centers.data_ptr(), knn.data_ptr(),
                                                             ops._p(cidx), c.B, c.rep, c.N, c.G, c.K, c.C, float(c.radius), out.data_ptr(), ws, n, s())
        elif isinstance(c, BC.UpscaleCase):
            keys, hyper, idx3, w3 = cu(inp["keys"].reshape(c.Z * c.G, c.dim)), cu(inp["hyper"]), cu(inp["idx3"]), cu(inp["w3"])
            buf, flat = padded(c.Z * c.C, c.N)
            masks = flat.view(c.Z, c.C, c.N)
            self.keep = (keys, hyper, idx3, w3)
            self.bufs, self.outs, self.reset = [(buf, c.Z * c.C)], [masks], lambda: masks.fill_(-7.0)
            self.need = int(lib.psam_upscale_masks_ws_bytes(c.Z, c.N, c.G, c.C, stage.dim))
            self.call = lambda ws, n: lib.psam_upscale_masks(ctypes.byref(stage.plan), stage.blob.data_ptr(), keys.data_ptr(), idx3.data_ptr(), w3.data_ptr(), hyper.data_ptr(), c.rep,
                                                             c.Z, c.N, c.G, c.C, masks.data_ptr(), ws, n, s())
        else:
            R, I = c.Z * c.T, c.Z * c.G
            tokens, keys0, pos = cu(inp["tokens"].reshape(R, c.E)), cu(inp["keys"].reshape(I, c.E)), cu(inp["pos"])
            qbuf, queries = padded(R, c.E)
            kbuf, keys = padded(I, c.E)
            self.keep = (tokens, keys0, pos)
            self.bufs, self.outs = [(qbuf, R), (kbuf, I)], [queries, keys]

            def reset():
                keys.copy_(keys0)
                queries.fill_(-7.0)
            self.reset = reset
            self.need = int(lib.psam_twoway_decoder_ws_bytes(c.Z, c.T, c.G, c.E, c.mlp))
            cnt = ops.arrival_counters(tokens.device).data_ptr() if c.counters else None
            self.call = lambda ws, n: lib.psam_twoway_decoder(ctypes.byref(stage.plan), stage.blob.data_ptr(), tokens.data_ptr(), keys.data_ptr(), pos.data_ptr(), c.rep, c.Z, c.T, c.G,
                                                              queries.data_ptr(), ws, n, cnt, s())

    def run(self):
        """The call on a workspace of its own -> clones of the outputs."""
        ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")
        self.reset()
        status = self.call(ws.data_ptr(), ws.numel())
        assert status == 0, (status, self.lib.psam_last_error_string().decode())
        torch.cuda.synchronize()
        return [t.clone() for t in self.outs]

    def sentinels_kept(self):
        return all(bool((buf[rows:] == SENT).all()) for buf, rows in self.bufs)


def case_id(c):
    return "-".join(str(v) for f, v in zip(c._fields, c) if f not in ("want", "refused", "seed", "cin")).replace(" ", "_")


def problem_of(ops, c):
    """Weights, inputs, fp64 outputs and e32 of the case; the 3-NN plan of an upscaling case comes from ops.three_nn on the case's random points."""
    if isinstance(c, BC.UpscaleCase):
        inp = BR.case_inputs(c)
        idx3, w3 = ops.three_nn(inp["xyz"].cuda(), inp["centers"].cuda())
        assert int(idx3.min()) >= 0 and int(idx3.max()) < c.G
        return BR.problem(c, idx3.cpu(), w3.cpu())
    return BR.problem(c)


def check_case(ops, stages, c):
    lib = ops._lib.load()
    _, inp, y64, e32 = problem_of(ops, c)
    r = Runner(ops, c, stages(c), inp)
    mode = getattr(c, "mode", -1)
    try:
        if mode >= 0:
            lib.psam_twoway_decoder_force_fast(mode)
        got = r.run()
        if isinstance(c, BC.TwowayCase):      # the final attention is the last one launched
            assert lib.psam_attention_small_last_instance() == c.want[6], "psam_attention_small ran another kernel than the case names"
        # 1. accuracy against fp64, measured in units of the fp32 oracle's own error
        bad = []
        for i, (y, want, e0) in enumerate(zip(got, y64, e32)):
            assert y.shape == want.shape and torch.isfinite(y).all()
            e = BR.rel_err(y, want)
            print(f"\n[ratio] {r.entry} | {case_id(c)} | out{i} | e_gpu {e:.3e} | e32 {e0:.3e} | ratio {e / e0:.2f}")
            if not e <= C_BOUND * e0 + 1e-7:
                bad.append((i, e, e0, e / e0))
        assert not bad, f"{r.entry} {case_id(c)}: (output, e_gpu, e32, ratio) {bad} over {C_BOUND} x e32 + 1e-7"
        # 2. repeatable
        again = r.run()
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "the same call twice: other bits"
        # 3. exactly *_ws_bytes, between guards
        check_exact_workspace(r.need, r.call, r.reset, lambda: r.outs, got)
        # 4. rows past the end
        assert r.sentinels_kept(), "rows behind the output were written"
    finally:
        if mode >= 0:
            lib.psam_twoway_decoder_force_fast(-1)


def check_refused(ops, stages, c):
    lib = ops._lib.load()
    entry = {BC.EvaCase: "psam_eva_block", BC.GeluCase: "psam_eva_gelu_block", BC.PatchCase: "psam_patch_encoder", BC.UpscaleCase: "psam_upscale_masks",
             BC.TwowayCase: "psam_twoway_decoder"}[type(c)]
    if c.refused == "prepare":
        sd = {n: t.cuda().contiguous() for n, t in BR.case_weights(c).items()}
        base = {BC.EvaCase: ops.EvaBlock, BC.GeluCase: ops.EvaGeluBlock, BC.PatchCase: ops.CPatchEncoder, BC.UpscaleCase: ops.CUpscale, BC.TwowayCase: ops.CTwoWay}[type(c)]
        status, msg, untouched = build_stage(ops, c, sd, cls=lambda *a: raw_prepare(ops, base, *a))
        assert status == EINVAL and msg.startswith(entry + "_prepare:") and untouched, (status, msg, untouched)
        return
    inp = BR.case_inputs(c)
    if isinstance(c, BC.UpscaleCase):
        inp["idx3"], inp["w3"] = ops.three_nn(inp["xyz"].cuda(), inp["centers"].cuda())
    r = Runner(ops, c, stages(c), inp)
    ws = torch.full((max(r.need, 1 << 20),), 0xA5, dtype=torch.uint8, device="cuda")
    r.reset()
    before = [t.clone() for t in r.outs]
    status = r.call(ws.data_ptr(), ws.numel())
    msg = lib.psam_last_error_string().decode()
    torch.cuda.synchronize()
    assert status == EINVAL and msg.startswith(entry + ":"), (status, msg)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(r.outs, before)) and r.sentinels_kept(), "a refused call wrote an output"
    assert bool((ws == 0xA5).all()), "a refused call wrote its workspace: something was launched"


ids = lambda cases: [case_id(c) for c in cases]


@pytest.mark.parametrize("case", BC.EVA_CASES, ids=ids(BC.EVA_CASES))
def test_eva_block(ops, stages, case):
    """psam_eva_block: Hp != H (zero gate rows, stat_cols < Hp) and Hp == H, 3 * dim an odd number of column tiles, one key per cloud, L no multiple of
    the key tile, heavy-tailed weights on the a-priori bounds (qkv_bound, v_bound, u_c0..2)."""
    check_case(ops, stages, case)


@pytest.mark.parametrize("case", BC.GELU_CASES, ids=ids(BC.GELU_CASES))
def test_eva_gelu_block(ops, stages, case):
    """psam_eva_gelu_block: head dims 64 / 72 / 88 / 128, the fused and the unfused fc1 -> fc2 hand-over (by the rows and by the hidden width), M no multiple
    of 256, one key per cloud, the key-split attention of a single cloud (cap 1 and 4), with and without the arrival counters."""
    check_case(ops, stages, case)


@pytest.mark.parametrize("case", BC.PATCH_CASES, ids=ids(BC.PATCH_CASES))
def test_patch_encoder(ops, stages, case):
    """psam_patch_encoder: every h1 / cout, groups of 32 / 64 / 128 / 192 (1, 2, 3 pooled parts; the partial maxima in recycled buffers), the pooled half
    on the row kernel and on the packed GEMM, C 1 / 3, with and without centre features and radius, two mask sets per cloud."""
    check_case(ops, stages, case)


@pytest.mark.parametrize("case", BC.UPSCALE_CASES, ids=ids(BC.UPSCALE_CASES))
def test_upscale_masks(ops, stages, case):
    check_case(ops, stages, case)


@pytest.mark.parametrize("case", BC.TWOWAY_CASES, ids=ids(BC.TWOWAY_CASES))
def test_twoway_decoder(ops, stages, case):
    """psam_twoway_decoder on each side of R <= 64, R >= 256, I >= 256, G <= 2048, T <= 16 and at the key limit, in its three launch sequences, without
    counters, at depth 1, downsample 1 / 4 and E = 128: both outputs, `queries` and the updated `keys`."""
    check_case(ops, stages, case)


REFUSED = BC.EVA_REFUSED + BC.GELU_REFUSED + BC.PATCH_REFUSED + BC.UPSCALE_REFUSED + BC.TWOWAY_REFUSED


@pytest.mark.parametrize("case", REFUSED, ids=[type(c).__name__ + "-" + case_id(c) for c in REFUSED])
def test_refused_before_the_first_launch(ops, stages, case):
    check_refused(ops, stages, case)


def test_supported_agrees_with_prepare(ops):
    """ops.EvaBlock / EvaGeluBlock / CPatchEncoder.supported(...) is true exactly when *_prepare returns 0 (prepare allocates: hence the GPU)."""
    dev = lambda sd: {n: t.cuda().contiguous() for n, t in sd.items()}
    for dim, heads, hidden in BC.SUPPORTED_GRID:
        st, msg, _ = raw_prepare(ops, ops.EvaBlock, dev(BR.eva_weights(dim, hidden, 1)), BR.BLK, dim, heads, hidden, BR.EVA_EPS)
        assert (st == 0) == ops.EvaBlock.supported(dim, heads, hidden) and st in (0, EINVAL), ("psam_eva_block", dim, heads, hidden, st, msg)
        st, msg, _ = raw_prepare(ops, ops.EvaGeluBlock, dev(BR.gelu_weights(dim, hidden, 1)), BR.BLK, dim, heads, hidden, BR.EVA_EPS)
        assert (st == 0) == ops.EvaGeluBlock.supported(dim, heads, hidden) and st in (0, EINVAL), ("psam_eva_gelu_block", dim, heads, hidden, st, msg)
    for h0, h1, cout in BC.PATCH_GRID:
        st, msg, _ = raw_prepare(ops, ops.CPatchEncoder, dev(BR.patch_weights(6, h0, h1, cout, 1)), BR.PATCH, BR.LN_EPS)
        assert (st == 0) == ops.CPatchEncoder.supported(h0, h1, cout) and st in (0, EINVAL), ("psam_patch_encoder", h0, h1, cout, st, msg)
