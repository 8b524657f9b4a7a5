"""Named inputs for psam_linear128_ln_gelu_pack (csrc/patch_rowln.hip), known bit for bit without a GPU: the operands are packed on the CPU
(g8_reference.row_scale_f16 / pack_g8 yield the device's containers), and the fp64 result is taken on the exactly decoded operands -- the formula of
test_gpu_patch_rowln.py's _inputs.  test_patch_rowln_cases_cpu.py asserts that every case has the property it is named for; test_gpu_patch_rowln_edges.py
runs them.  `place` puts a case on the device inside padded, guarded storage."""
import functools
import math
import types

import torch

from g8_reference import pack_g8, row_scale_f16, unpack_g8

H0, H1, EPS = 128, 512, 1e-5
NAN_WORD = 0x7FC07FC0                  # a NaN as one fp32 and as each of its two fp16 halves: what fills the padding of every input
GUARD_WORD = 0xA5A5A5A5 - (1 << 32)    # what fills the storage around (and the padding columns of) out and out_scale
GUARD_WORDS = 1024                     # 4 KiB on each side
NAN_ROW = 77                           # the row that "a non-finite row" replaces

# name -> (rows, rowgroup, kind).  A seed per name (its position here), never changed.
#   plain              gamma and beta clamped, so that the bound stays below 32 (the scale test moves it across that power of two)
#   rowgroup G         rows = the smallest multiple of 64 and G with at least three blocks; with G = 96 and 160 a bias row changes at an odd 32-row tile
#   one bias row       rowgroup = rows: what a row permutation leaves alone
#   variance near eps  zero bias rows, every row of x scaled so that var(y) = eps f, f log-uniform in [1/2, 2]
#   row magnitudes     row maxima of x = 2^e, e from -60 to 40 in a shuffled order, ordinary bias rows
#   gamma outlier      the "special" construction of test_gpu_patch_rowln.py: a block of zero rows, one input 1e4 x its row, gamma[13] x 50
CASES = {
    "plain": (256, 64, "plain"),
    "one block": (64, 64, "plain"),
    "rowgroup 64": (192, 64, "plain"),
    "rowgroup 96": (192, 96, "plain"),
    "rowgroup 128": (256, 128, "plain"),
    "rowgroup 160": (320, 160, "plain"),
    "rowgroup 256": (256, 256, "plain"),
    "one bias row": (256, 256, "plain"),
    "variance near eps": (256, 64, "var_eps"),
    "row magnitudes": (256, 64, "magnitudes"),
    "gamma outlier": (256, 64, "special"),
}
NAMES = list(CASES)


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def row_ln_bound(gamma, beta):
    """ops.row_ln_bound, on the CPU."""
    return float((gamma.numel() - 1) ** 0.5 * gamma.abs().max().item() + beta.abs().max().item())


def reference(xp, sx, wp, sw, g1, rowgroup, gamma, beta, eps=EPS):
    """(fp64 result, per-row variance of y) on the exactly decoded packed operands: mean, biased variance, eps, erf GELU."""
    y = unpack_g8(xp, sx, H0) @ unpack_g8(wp, sw, H0).T + g1.double().repeat_interleave(rowgroup, dim=0)
    mu = y.mean(dim=1, keepdim=True)
    var = ((y - mu) ** 2).mean(dim=1, keepdim=True)
    return gelu64((y - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()), var[:, 0]


def _pack(c):
    c["sx"], c["sw"] = row_scale_f16(c["x"]), row_scale_f16(c["W"])
    c["xp"], c["wp"] = pack_g8(c["x"], c["sx"]), pack_g8(c["W"], c["sw"])
    return c


def cyclic_permutation(n, seed):
    """A permutation of one n-cycle in a random order: it fixes no row."""
    order = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    perm = torch.empty(n, dtype=torch.int64)
    perm[order] = order.roll(-1)
    return perm


@functools.lru_cache(maxsize=None)
def build(name):
    """The case as CPU tensors -- built once, shared, never written."""
    rows, K, kind = CASES[name]
    g = torch.Generator().manual_seed(7000 + NAMES.index(name))
    x = torch.randn(rows, H0, generator=g) * torch.exp(0.5 * torch.randn(rows, 1, generator=g))
    W = torch.randn(H1, H0, generator=g) / 11
    gamma, beta = 1.0 + 0.1 * torch.randn(H1, generator=g), 0.1 * torch.randn(H1, generator=g)
    g1 = torch.randn(rows // K, H1, generator=g)
    if kind == "plain":
        gamma, beta = gamma.clamp(0.7, 1.3), beta.clamp(-0.3, 0.3)      # bound <= 1.001 (sqrt(511) 1.3 + 0.3) < 29.8
    elif kind == "special":
        x[:64] = 0.0; g1[0] = 0.0
        x[100, 7] *= 1e4
        gamma[13] *= 50.0
    elif kind == "var_eps":
        g1.zero_()
        var = (x.double() @ W.double().T).var(dim=1, unbiased=False)
        f = torch.exp2(2.0 * torch.rand(rows, generator=g, dtype=torch.float64) - 1.0)
        x = (x.double() * torch.sqrt(EPS * f / var)[:, None]).float()      # (the packing then moves var(y) by a relative 2^-21 or so)
    elif kind == "magnitudes":
        e = torch.linspace(-60.0, 40.0, rows, dtype=torch.float64)[torch.randperm(rows, generator=g)]
        x = (x.double() / x.double().abs().amax(dim=1, keepdim=True) * torch.exp2(e)[:, None]).float()
    c = _pack(dict(name=name, rows=rows, rowgroup=K, eps=EPS, x=x, W=W, gamma=gamma, beta=beta, g1=g1))
    c["bound"] = 1.001 * row_ln_bound(gamma, beta) + 1e-30
    c["want"], c["var"] = reference(c["xp"], c["sx"], c["wp"], c["sw"], g1, K, gamma, beta)
    if name == "one bias row":
        c["perm"] = cyclic_permutation(rows, 7100)
    return c


def with_nan_row(c, row=NAN_ROW):
    """The case with one row of x replaced by NaNs and packed again by the reference (scale 1, NaN in every hi and lo half); no fp64 result."""
    x = c["x"].clone()
    x[row] = float("nan")
    d = _pack(dict(c, x=x))
    d.pop("want"); d.pop("var")
    return d


def trip_case(nblocks, seed=7200):
    """Operands for nblocks 64-row blocks under rowgroup = 64, from one cheap generator and with no fp64 result (`head` takes the smaller sizes from it)."""
    g = torch.Generator().manual_seed(seed)
    rows = 64 * nblocks
    W = torch.randn(H1, H0, generator=g) / 11
    gamma, beta = (1.0 + 0.1 * torch.randn(H1, generator=g)).clamp(0.7, 1.3), (0.1 * torch.randn(H1, generator=g)).clamp(-0.3, 0.3)
    x = torch.randn(rows, H0, generator=g)
    g1 = torch.randn(nblocks, H1, generator=g)
    c = _pack(dict(name=f"{nblocks} blocks", rows=rows, rowgroup=64, eps=EPS, x=x, W=W, gamma=gamma, beta=beta, g1=g1))
    c["bound"] = 1.001 * row_ln_bound(gamma, beta) + 1e-30
    return c


def head(c, nblocks):
    """The first nblocks 64-row blocks of a rowgroup-64 case."""
    assert c["rowgroup"] == 64 and 64 * nblocks <= c["rows"]
    rows = 64 * nblocks
    return dict(c, name=f"{nblocks} blocks", rows=rows, x=c["x"][:rows], xp=c["xp"][:rows], sx=c["sx"][:rows], g1=c["g1"][:nblocks])


# ---- on the device

def _padded(t, ld, device):
    """[r, c] 32-bit CPU tensor -> its bits as an fp32 view [r, c] of a [r, ld] device buffer whose other columns hold NAN_WORD."""
    r, cols = t.shape
    buf = torch.full((r, ld), NAN_WORD, dtype=torch.int32)
    buf[:, :cols] = t.contiguous().view(torch.int32)
    return buf.to(device).view(torch.float32)[:, :cols]


def _carved(n, device):
    """n words exactly between two guards of GUARD_WORDS -> (the whole int32 buffer, the n words)."""
    buf = torch.full((n + 2 * GUARD_WORDS,), GUARD_WORD, dtype=torch.int32, device=device)
    return buf, buf[GUARD_WORDS:GUARD_WORDS + n]


def place(c, ldx=H0, ldw=H0, ldrb=H1, ldo=H1, arena=False, device="cuda"):
    """The operands of a case on the device, rows of x, W, g1 and out at the given leading dimensions (views into wider buffers whose padding columns
    hold NaNs, for out the guard word).  out [rows, ldo] and out_scale [rows] are carved exactly out of guard words (`guards_intact`).
    arena=True: x_scale, g1, gamma, beta and w_scale lie in ONE NaN-filled arena, each at its alignment (4 bytes for x_scale, 16 for the rest) with no
    more than that alignment's worth of NaNs between one's last element and the next one's first, so a read one element past (or before) any of them
    is a NaN."""
    rows = c["rows"]
    d = types.SimpleNamespace(rows=rows)
    d.x = _padded(c["xp"], ldx, device)
    wpk = _padded(c["wp"], ldw, device)
    if arena:
        assert ldrb == H1
        parts = dict(sx=c["sx"], g1=c["g1"], gamma=c["gamma"], beta=c["beta"], sw=c["sw"])
        gap, at, off = 4, {}, 4
        for k, t in parts.items():
            at[k] = off
            off += (t.numel() + gap + 3) // 4 * 4
        buf = torch.full((off,), NAN_WORD, dtype=torch.int32)
        for k, t in parts.items():
            buf[at[k]:at[k] + t.numel()] = t.contiguous().view(torch.int32).reshape(-1)
        d.arena = buf.to(device).view(torch.float32)
        for k, t in parts.items():
            setattr(d, k, d.arena[at[k]:at[k] + t.numel()].view(t.shape))
    else:
        d.sx, d.sw, d.gamma, d.beta = c["sx"].to(device), c["sw"].to(device), c["gamma"].to(device), c["beta"].to(device)
        d.g1 = _padded(c["g1"], ldrb, device)
    d.fw = types.SimpleNamespace(packed=wpk, scale=d.sw, N=H1)
    d.out_buf, o = _carved(rows * ldo, device)
    d.out = o.view(torch.float32).view(rows, ldo)[:, :H1]
    d.rs_buf, r = _carved(rows, device)
    d.rs = r.view(torch.float32)
    d.ldo = ldo
    return d


def guards_intact(d):
    """Every word of out's and out_scale's buffers outside out[:, :512] and out_scale still holds the guard word."""
    o = d.out_buf.clone()
    o[GUARD_WORDS:GUARD_WORDS + d.rows * d.ldo].view(d.rows, d.ldo)[:, :H1] = GUARD_WORD
    r = d.rs_buf.clone()
    r[GUARD_WORDS:GUARD_WORDS + d.rows] = GUARD_WORD
    return bool((o == GUARD_WORD).all()) and bool((r == GUARD_WORD).all())
