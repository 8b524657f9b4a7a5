"""The "g8" packed-row format of the f16x3 path, stated once for the tests (the device side is point_sam_amd/csrc/g8_pack.h).

A row x[0 .. K) with its power-of-two scale s is stored in 32-bit containers, Kp = K rounded up to 32 of them: for each group of 8 consecutive columns,
containers 8g .. 8g+3 hold hi = RNE_fp16(s * x) (two columns per container, the lower column in the low half-word) and containers 8g+4 .. 8g+7 hold
lo = RNE_fp16(s * x - hi).  Columns K .. Kp - 1 are zeros.  Plain torch; `pack_g8` runs on the CPU with the operations of the device split (one fp32
product, which is exact for a power-of-two scale short of overflow; round to nearest even; an exact fp32 residual), so it yields the device's containers."""
import torch


def kpad32(K):
    return (K + 31) // 32 * 32


def row_scale_f16(x):
    """[rows, K] fp32 -> [rows] fp32: 2^(14 - e), e = floor(log2(row maximum of |x|)) clamped below at -112; 1 for an all-zero or non-finite row
    (f16_row_scale of csrc/common.h, on the exponent bits)."""
    bits = x.detach().cpu().float().abs().amax(dim=1).contiguous().view(torch.int32)
    e = ((bits >> 23) & 0xFF) - 127
    scale = (((127 + 14) - e.clamp(min=-112)) << 23).to(torch.int32).view(torch.float32)
    return torch.where((bits == 0) | (e == 128), torch.ones_like(scale), scale)


def pack_g8(x, scale):
    """[rows, K] fp32, [rows] fp32 power-of-two scales -> [rows, kpad32(K)] int32 containers."""
    x, scale = x.detach().cpu().float(), scale.detach().cpu().float()
    rows, K = x.shape
    Kp = kpad32(K)
    xs = torch.zeros(rows, Kp)
    xs[:, :K] = x * scale[:, None]
    hi = xs.to(torch.float16)                       # round to nearest even
    lo = (xs - hi.float()).to(torch.float16)        # the residual is exact in fp32
    halves = torch.stack([hi.view(rows, Kp // 8, 8), lo.view(rows, Kp // 8, 8)], dim=2)      # [rows, group, hi | lo, 8]
    return halves.contiguous().view(rows, Kp * 2).view(torch.int32)


def unpack_g8(p, scale, K):
    """[rows, Kp] g8-packed containers -> (hi + lo) / scale as fp64 [rows, K] (the inverse of the packing), on the device of `p`."""
    rows, Kp = p.shape
    h = p.contiguous().view(torch.float16).view(rows, Kp // 8, 2, 8).double()        # [rows, group, hi|lo, 8]
    return ((h[:, :, 0] + h[:, :, 1]).reshape(rows, Kp) / scale.double()[:, None])[:, :K]
