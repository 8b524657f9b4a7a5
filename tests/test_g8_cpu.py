"""The g8 packed-row format without a GPU: the host packer of tests/g8_reference.py against the format's definition, and the rule that csrc/g8_pack.h is the
only file of the library that writes it."""
import os
import re

import pytest
import torch

import g8_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point_sam_amd", "csrc")


def _rows(rows, K, seed):
    """Rows with magnitudes spread over 2^+-40 (between rows and, by 2^-20 .. 1, inside a row) and exact zeros sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g) * 2.0 ** -torch.randint(0, 21, (rows, K), generator=g).float()
    x = x * 2.0 ** torch.randint(-40, 41, (rows, 1), generator=g).float()
    x[torch.rand(rows, K, generator=g) < 0.1] = 0.0
    return x


@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("K", [4, 36, 260, 516])
def test_host_packer_round_trip_padding_and_hi(rows, K):
    """unpack_g8(pack_g8(x, s), s) is x to 2^-21 of the row maximum (hi + lo = 22 significand bits); the padding columns are zero; hi is the RNE fp16 of
    s * x, in the containers the layout names: group g at 8g .. 8g+3, two columns per container, the lower column in the low half-word."""
    x = _rows(rows, K, seed=rows * 1000 + K)
    s = G.row_scale_f16(x)
    amax = x.abs().amax(1)
    assert ((s * amax >= 2.0 ** 14) & (s * amax < 2.0 ** 15) | (amax == 0)).all()
    p = G.pack_g8(x, s)
    Kp = G.kpad32(K)
    assert p.shape == (rows, Kp) and p.dtype == torch.int32 and Kp % 32 == 0 and 0 <= Kp - K < 32
    dec = G.unpack_g8(p, s, Kp)
    assert (dec[:, K:] == 0).all() and (p[:, (K + 7) // 8 * 8:] == 0).all()
    rel = (dec[:, :K] - x.double()).abs() / x.double().abs().amax(1, keepdim=True).clamp(min=1e-300)
    assert rel.max().item() <= 2.0 ** -21, rel.max().item()
    hi = (x * s[:, None]).to(torch.float16)
    for c in range(K):
        word = p[:, c // 8 * 8 + (c % 8) // 2]
        half = ((word >> 16) if c % 2 else word) & 0xFFFF
        assert torch.equal(half.to(torch.int16), hi[:, c].view(torch.int16)), c


def test_host_packer_zero_and_infinite_rows():
    """A row of zeros and a row with an infinity have scale 1; the zero row packs to zero words, the infinity stays an fp16 infinity in its hi half."""
    x = _rows(5, 36, seed=3)
    x[1] = 0.0
    x[3, 7] = float("inf")
    s = G.row_scale_f16(x)
    assert s[1] == 1.0 and s[3] == 1.0 and (s[[0, 2, 4]] != 1.0).all()
    p = G.pack_g8(x, s)
    assert (p[1] == 0).all()
    assert (p[3, 3] >> 16) & 0xFFFF == 0x7C00                      # column 7: container 3 of group 0, high half
    keep = [r for r in range(5) if r != 3]
    dec = G.unpack_g8(p[keep], s[keep], 36)
    assert ((dec - x[keep].double()).abs() <= 2.0 ** -21 * x[keep].double().abs().amax(1, keepdim=True)).all()


def test_the_g8_layout_lives_in_one_header():
    """csrc/g8_pack.h is the only file that splits a scaled value with its row scale, assembles a parity-selected chunk or exchanges half-words for one
    (experiments/ aside); the files that pack include it; the attention kernels' private copies of the split and of inv_pow2 are gone."""
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".cpp"))}
    where = lambda pat: [f for f, src in sources.items() if re.search(pat, src)]
    assert where(r"psam_split2_f16\(") == ["g8_pack.h"]
    assert where(r"g8_split2_scaled\(") == ["attention.hip", "g8_pack.h"]           # the key loop's fragment builders keep the pre-scaled form
    assert where(r"\?\s*\w*u32x4\s*\{") == ["g8_pack.h"]                            # upper ? {r0, r1, l0, l1} : {h0, h1, r0, r1}
    assert where(r"typedef\s+unsigned\s+\w*u32x4\b") == ["g8_pack.h"]
    assert where(r"permlane32_swap\(") == ["common.h"]
    assert where(r"psam_swap32\(") == ["common.h", "g8_pack.h", "gemm_epilogue_t.h"]   # the epilogue's segment sums exchange floats, never half-words
    assert "psam_swap32(" not in sources["gemm_epilogue_t.h"].replace("psam_swap32(x, y);", "", 1)
    assert where(r"__shfl_xor\([^;\n]*\b[hl][01]\b") == ["g8_pack.h"]               # no half-word goes through a lane shuffle outside the header
    assert where(r"\b(fa_split2|fa_inv_pow2)\b") == []
    assert where(r"float inv_pow2\(") == ["common.h"] and where(r"int kpad32\(") == ["g8_pack.h"]
    assert where(r"\+ 31\) / 32 \* 32|\+ 31\) & ~31") == ["g8_pack.h"]
    for f in ("rowops.hip", "attention.hip", "tokenizer.hip", "gemm_f16x3p.hip", "blocks.hip", "gemm_epilogue.h", "gemm_f16x3p_args.h"):
        assert '#include "g8_pack.h"' in sources[f], f
    assert '#include "gemm_epilogue.h"' in sources["gemm_epilogue_t.h"] and '#include "gemm_epilogue_t.h"' in sources["gemm_f16x3pp.hip"]
    # the writers, by the one function each calls
    calls = {"g8_chunk<1>(": ["gemm_epilogue.h", "gemm_f16x3p.hip", "rowops.hip"], "g8_chunk<1, true>(": ["gemm_f16x3p.hip", "rowops.hip"],
             "g8_chunk_scaled<32>(": ["attention.hip"],
             "g8_halfwave_group(": ["g8_pack.h", "gemm_epilogue_t.h"], "g8_whole_group(": ["g8_pack.h", "gemm_f16x3p.hip"],
             "g8_store_pair(": ["g8_pack.h", "tokenizer.hip"]}
    for call, files in calls.items():
        assert sorted(f for f, src in sources.items() if call in src) == sorted(files), call
    assert sources["gemm_epilogue_t.h"].count("g8_halfwave_group(") == 2 and sources["attention.hip"].count("g8_chunk_scaled<32>(") == 2
    assert sources["rowops.hip"].count("g8_chunk<1>(") == 2 and sources["gemm_f16x3p.hip"].count("g8_chunk<1>(") == 2
    assert sources["rowops.hip"].count("g8_chunk<1, true>(") == 1 and sources["gemm_f16x3p.hip"].count("g8_chunk<1, true>(") == 1
