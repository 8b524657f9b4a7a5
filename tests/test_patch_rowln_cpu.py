"""psam_linear128_ln_gelu_pack (csrc/patch_rowln.hip) refuses on the host, before any launch, with the library's status codes: no GPU needed (the
pointers below are never dereferenced)."""
from point_sam_amd import _lib

EINVAL, EALIGN = -1, -2
P = 0x10000      # any 32-byte aligned non-null address


def _call(lib, x=P, ldx=128, sx=P, w=P, ldw=128, sw=P, rowbias=P, ldrb=512, rowgroup=64, gamma=P, beta=P, rows=256, h1=512, out=P, ldo=512, rs=P):
    return lib.psam_linear128_ln_gelu_pack(x, ldx, sx, w, ldw, sw, rowbias, ldrb, rowgroup, gamma, beta, 1e-5, 30.0, rows, h1, out, ldo, rs, None)


def test_linear128_ln_gelu_pack_refuses_before_the_first_launch():
    lib = _lib.load()
    for name in ("x", "sx", "w", "sw", "rowbias", "gamma", "beta", "out", "rs"):
        assert _call(lib, **{name: None}) == EINVAL, name
        assert b"null pointer" in lib.psam_last_error_string()
    for h1 in (256, 384, 511, 1024):
        assert _call(lib, h1=h1) == EINVAL, h1
    assert b"512 columns" in lib.psam_last_error_string()
    for rows in (0, -64, 32, 100, 257, 1 << 31, (1 << 31) + 64, 1 << 40):
        assert _call(lib, rows=rows) == EINVAL, rows
    assert b"multiple of 64" in lib.psam_last_error_string()
    for kw in (dict(rowgroup=0), dict(rowgroup=-32), dict(rowgroup=16), dict(rowgroup=48), dict(ldx=96), dict(ldw=64), dict(ldrb=256), dict(ldo=256)):
        assert _call(lib, **kw) == EINVAL, kw
    for kw in (dict(x=P + 16), dict(w=P + 4), dict(out=P + 8), dict(ldx=132), dict(ldw=129), dict(ldo=516), dict(rowbias=P + 4), dict(gamma=P + 8), dict(beta=P + 12),
               dict(sw=P + 4), dict(ldrb=514)):
        assert _call(lib, **kw) == EALIGN, kw
    assert b"aligned" in lib.psam_last_error_string()
    assert _call(lib, rows=(1 << 31) - 64, x=None) == EINVAL      # the largest row count it takes is refused for its null pointer only
    assert b"null pointer" in lib.psam_last_error_string()
