"""Hand-made inputs for the voxel normals (csrc/normals.hip) where the scatter matrix S = n P - s s^T does not fit fp64, where its conversion to fp64
sits on a rounding edge, and where the eigen solve has no eigenvalue gap.  Plain numpy and Python integers; nothing here needs a GPU.

Every case is (xyz [N, 3] f32, inv [N] int64, nbr [V, 26] int32), the arguments of ops.voxel_normals and of superpoint_reference.scatter.  The cases
built from integers use V = 1, inv = 0 and nbr = -1: the whole cloud is one neighbourhood, and a fixed-point value q in [0, 2^21] becomes the
coordinate p = q * 2^-20 - 1, exact in fp32 (21 significant bits at most), which floor(p * 2^20) + 2^20 takes back to q."""
import random

import numpy as np

ONE = 1 << 20
f32 = np.float32


def from_fixed(q, seed=0):
    """Integer fixed-point values q [N, 3] in [0, 2^21] -> one neighbourhood holding exactly these points, shuffled."""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 3)
    assert q.min() >= 0 and q.max() <= 2 * ONE
    xyz = (q.astype(np.float64) / ONE - 1.0).astype(f32)
    assert np.array_equal(np.floor(xyz.astype(np.float64) * ONE).astype(np.int64) + ONE, q), "p = q 2^-20 - 1 is exact in fp32"
    xyz = xyz[np.random.default_rng(seed).permutation(len(xyz))]
    return np.ascontiguousarray(xyz), np.zeros(len(xyz), dtype=np.int64), np.full((1, 26), -1, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ a chosen product in every entry of S
def two_cluster(m, d):
    """m copies of a point u and m copies of a point w with w - u = d (three integers, |d_a| <= 2^21); per axis u_a = 0, w_a = d_a, or for a
    negative d_a the two ends swapped: u_a = -d_a, w_a = 0.  Then, exactly, S_ab = m^2 d_a d_b:

        n = 2 m,   s_a = m (u_a + w_a),   P_ab = m (u_a u_b + w_a w_b)
        S_ab = n P_ab - s_a s_b = m^2 (2 u_a u_b + 2 w_a w_b - (u_a + w_a)(u_b + w_b)) = m^2 (u_a - w_a)(u_b - w_b) = m^2 d_a d_b

    so any product of that shape, with its sign, can be put into the xy entry with N = 2 m points."""
    d = [int(c) for c in d]
    assert m >= 1 and len(d) == 3 and all(abs(c) <= 2 * ONE for c in d)
    u = [max(-c, 0) for c in d]
    w = [max(c, 0) for c in d]
    return from_fixed(np.array([u] * m + [w] * m, dtype=np.int64), seed=m)


def two_cluster_scatter(m, d):
    """The six exact entries xx, xy, xz, yy, yz, zz of two_cluster(m, d)."""
    return [m * m * int(d[a]) * int(d[b]) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]


# ------------------------------------------------------------------------------------------------ where float(S) rounds
def pattern(x):
    """The rounding edge |x| sits on when it is rounded to 53 bits, or None.  b = |x|.bit_length(), kept = |x| >> (b - 53):

        'tie_even'     the low b - 53 bits are exactly half a unit of kept, kept even: to nearest even the value stays at kept
        'tie_odd'      the same with kept odd: the value goes up
        'half_sticky'  b > 64: bit b - 54 set, bits b - 55 .. b - 64 clear, a bit below b - 64 set: above half, so up -- a conversion that drops the
                       bits shifted out of the top 64 sees a tie
        'below_half'   b > 64: bit b - 54 clear, bits b - 55 .. b - 64 all set, a bit below set: below half, so down -- a conversion that first
                       rounds to 64 bits may carry into a tie
        'below_half_odd'  below_half where that carry does happen (the bits below b - 64 are at least half a unit of the 64) and the tie it makes
                       is resolved the wrong way (kept is odd: up)"""
    x = abs(int(x))
    b = x.bit_length()
    if b <= 53:
        return None
    r = b - 53
    kept, low = x >> r, x & ((1 << r) - 1)
    if low == 1 << (r - 1):
        return "tie_odd" if kept & 1 else "tie_even"
    if b <= 64:
        return None
    t = b - 64                                                     # the bits below the top 64
    half, mid, rest = low >> (r - 1), (low >> t) & 1023, low & ((1 << t) - 1)
    if half == 1 and mid == 0 and rest != 0:
        return "half_sticky"
    if half == 0 and mid == 1023 and rest != 0:
        return "below_half_odd" if kept & 1 and rest >> (t - 1) else "below_half"
    return None


def search(m_bits, seed=5, draws=40000):
    """The first (m, d_x, d_y) per pattern of m^2 d_x d_y among `draws` draws of random.Random(seed): m in [2^m_bits[0], 2^m_bits[1]), d_x and d_y
    in [2^19, 2^21).  Deterministic, Python integers only."""
    rng = random.Random(seed)
    found = {}
    for _ in range(draws):
        m, dx, dy = rng.randrange(1 << m_bits[0], 1 << m_bits[1]), rng.randrange(1 << 19, 1 << 21), rng.randrange(1 << 19, 1 << 21)
        found.setdefault(pattern(m * m * dx * dy), (m, dx, dy))
    found.pop(None, None)
    return found


# What search((12, 14)) and search((7, 10)) return, as literals: (pattern, (m, d_x, d_y), bit length of m^2 d_x d_y).  Above 64 bits the conversion
# shifts, keeps a sticky bit and scales; up to 64 bits it is one u64 -> fp64 conversion, where only the ties exist.
HIGH = [("tie_even", (11168, 998948, 1559044), 68),
        ("tie_odd", (11168, 716046, 1183988), 67),
        ("below_half", (10826, 1735706, 1468774), 69),
        ("below_half_odd", (11329, 2082313, 1734413), 69),
        ("half_sticky", (13647, 2065831, 1988673), 70)]
LOW = [("tie_even", (314, 1340997, 859002), 57),
       ("tie_odd", (1020, 535430, 963549), 59)]
D_Z = 1234567                                                      # the third axis of every rounding case: odd, so xz and yz round somewhere else


def rounding_cases():
    """name -> (m, d): every committed triple, and each again with d_y negated (a negative xy entry)."""
    out = {}
    for kind, table in (("high", HIGH), ("low", LOW)):
        for name, (m, dx, dy), _ in table:
            out[f"{kind}_{name}"] = (m, (dx, dy, D_Z))
            out[f"{kind}_{name}_neg"] = (m, (dx, -dy, D_Z))
    return out


# ------------------------------------------------------------------------------------------------ wrong conversions, for the CPU tests
def _scaled(mant, shift):
    return float(mant) * 2.0 ** shift                              # mant < 2^54 and the power of two are exact, and so is their product here


def convert_truncating(x):
    """Keeps the top 53 bits."""
    s, x = (-1.0 if x < 0 else 1.0), abs(x)
    r = max(x.bit_length() - 53, 0)
    return s * _scaled(x >> r, r)


def convert_half_up(x):
    """Round to nearest, ties away from zero."""
    s, x = (-1.0 if x < 0 else 1.0), abs(x)
    r = max(x.bit_length() - 53, 0)
    return s * _scaled((x + ((1 << r) >> 1)) >> r, r)


def _nearest_even(x, r):
    """x / 2^r to the nearest integer, ties to even."""
    if r <= 0:
        return x
    q, low, half = x >> r, x & ((1 << r) - 1), 1 << (r - 1)
    return q + (1 if low > half or (low == half and q & 1) else 0)


def convert_twice(x):
    """Round to 64 bits, then to 53: each to nearest even."""
    s, x = (-1.0 if x < 0 else 1.0), abs(x)
    t = max(x.bit_length() - 64, 0)
    return s * float(_nearest_even(x, t)) * 2.0 ** t              # float(int) of at most 65 bits rounds once, to nearest even


def convert_without_sticky(x):
    """The top 64 bits to nearest even; the bits below them are dropped."""
    s, x = (-1.0 if x < 0 else 1.0), abs(x)
    t = max(x.bit_length() - 64, 0)
    return s * float(x >> t) * 2.0 ** t


WRONG = {"truncating": convert_truncating, "half_up": convert_half_up, "twice": convert_twice, "without_sticky": convert_without_sticky}


# ------------------------------------------------------------------------------------------------ neighbourhoods without an eigenvalue gap
def _lattice(steps, n=7, base=(ONE // 2, ONE // 2, ONE // 2)):
    """n^3 points base + i a + j b + k c for the three integer step vectors a, b, c."""
    i = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    return np.asarray(base, dtype=np.int64) + i @ np.asarray(steps, dtype=np.int64)


def _oblique_plane():
    """16 x 16 points on x + y + z = 3 * 2^20, step 512: base + 512 (i, j, -i - j)."""
    i, j = (g.ravel() for g in np.meshgrid(np.arange(16), np.arange(16), indexing="ij"))
    return np.array([ONE, ONE, ONE + 512 * 30]) + 512 * np.stack([i, j, -i - j], 1)


def degenerate_fixed():
    """name -> (q [N, 3] integers, spectrum): one token per ascending eigenvalue l0 <= l1 <= l2 of float(S) -- "0" zero, "e" positive but below
    1e-9 l2, and otherwise a letter: the same letter for equal eigenvalues ("a~": within 1 % of the other "a", not equal), another letter for one
    that is at least 0.1 l2 away."""
    t = np.arange(40, dtype=np.int64)[:, None]
    moved = _oblique_plane()
    moved[37, 0] += 1
    return {
        "coincident": (np.tile(np.array([123456, 654321, 1000000]), (50, 1)), ("0", "0", "0")),
        "line_x": (np.array([1000, 77777, 2000000]) + t * np.array([4096, 0, 0]), ("0", "0", "a")),
        "line_diagonal": (np.array([5000, 6000, 7000]) + t * np.array([3001, 3001, 3001]), ("0", "0", "a")),
        "line_skew": (np.array([ONE, ONE, ONE]) + t * np.array([3, -7, 11]), ("0", "0", "a")),
        "plane_oblique": (_oblique_plane(), ("0", "a", "b")),
        "cubic": (_lattice(np.diag([1000, 1000, 1000])), ("a", "a", "a")),
        "cubic_two_near": (_lattice(np.diag([1000, 1001, 3000])), ("a", "a~", "b")),
        "cubic_two_near_oblique": (_lattice([[600, 800, 0], [-800, 600, 1], [0, 3, 3000]]), ("a", "a~", "b")),
        "plane_oblique_one_moved": (moved, ("e", "a", "b")),                  # l0 is tiny and positive: one point is 1 / sqrt(3) steps off the plane
    }


def degenerate(name):
    return from_fixed(degenerate_fixed()[name][0], seed=len(name))


# ------------------------------------------------------------------------------------------------ the clouds of tests/test_gpu_superpoints.py
def plane(rng, n, axis, sigma):
    p = rng.uniform(-0.5, 0.5, (n, 3))
    p[:, axis] = -0.5 + rng.normal(0, sigma, n)
    return p


def cloud_points(name):
    """name -> (xyz [N, 3] fp64 or fp32, voxel size), from default_rng(sum(map(ord, name))): the same points on every call."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "box":                                     # three noisy planes meeting in a corner
        return np.concatenate([plane(rng, 2000, a, 0.002) for a in range(3)]), 0.05
    if name == "sphere":
        d = rng.normal(size=(6000, 3))
        return 0.7 * d / np.linalg.norm(d, axis=1, keepdims=True), 0.08
    if name == "uniform6000":
        return rng.uniform(-1, 1, (6000, 3)), 0.2
    if name == "uniform20000":                            # V well above 1024
        return rng.uniform(-1, 1, (20000, 3)), 0.09
    if name == "grid":                                    # an 80 x 80 lattice plane: coordinates are multiples of 2^-6, z is constant
        g = np.arange(-40, 40) / 64.0
        x, y = np.meshgrid(g, g, indexing="ij")
        return np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.125)], 1), 1.0 / 16
    if name == "edge":                                    # tests/test_gpu_regions.py's: points exactly at -1 on one, two or three axes
        xyz = rng.uniform(-1, 1, (1500, 3))
        for a in range(3):
            xyz[rng.choice(1500, 500, replace=False), a] = -1.0
        xyz[0] = -1.0
        return xyz, 0.125
    if name == "duplicates":                              # every point three times, shuffled
        base = rng.uniform(-1, 1, (700, 3)).astype(f32)
        return base[rng.permutation(np.repeat(np.arange(700), 3))], 0.17
    if name == "heavy":                                   # one voxel holds 5000 copies of a point near +1 (products near 2^42 each) and 10 others
        p = np.array([0.93, 0.97, 0.91])
        xyz = np.concatenate([np.tile(p, (5000, 1)), p + rng.uniform(-0.04, 0.02, (10, 3))])
        return xyz[rng.permutation(len(xyz))], 0.25
    if name.startswith("small"):                          # N = 63, 65, and 4 points in one neighbourhood (count < min_points everywhere)
        n = int(name[5:])
        return (rng.uniform(-0.1, 0.1, (n, 3)), 0.25) if n == 4 else (rng.uniform(-0.5, 0.5, (n, 3)), 0.25)
    if name == "large":                                   # 50^3 cells, ~62 % occupied: V > 70 000
        return rng.uniform(-1, 1, (120000, 3)), 0.04
    if name in WIDE:                                      # eight voxels, each other's neighbours: every neighbourhood is the whole cloud
        return rng.uniform(-1, 1, (WIDE[name], 3)), 1.0
    raise KeyError(name)


# Every |S| entry of the clouds above stays below 2^53 (checked in tests/test_superpoints_cpu.py); these two do not: with n points in one
# neighbourhood the diagonal of S is near n^2 2^40 / 3 and the rest near n^1.5 2^40 / 3.
#   wide    largest |S| 69 bits; 24 of the 48 entries (8 voxels x 6) above 64 bits, 48 not representable in fp64
#   wide18  75 bits, 40 of 48 above 64 bits (the xy entry has exactly 64), 48 not representable; 262144 points behind every word of the table
WIDE = {"wide": 1 << 15, "wide18": 1 << 18}
WIDE_COUNTS = {"wide": (69, 24, 48), "wide18": (75, 40, 48)}


def scatter_stats(S):
    """(bit length of the largest |S| entry, entries above 64 bits, entries float() does not represent) of the rows of exact integers S."""
    flat = [abs(x) for row in S for x in row]
    return max(flat).bit_length(), sum(x.bit_length() > 64 for x in flat), sum(float(x) != x for x in flat)
