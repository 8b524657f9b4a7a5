"""The cases of patch_rowln_cases.py have the properties they are named for, on the fp64 reference alone: no GPU needed."""
import math

import torch

import patch_rowln_cases as PC
from g8_reference import unpack_g8


def test_every_case_is_well_formed():
    for name, (rows, K, _) in PC.CASES.items():
        c = PC.build(name)
        assert 64 <= rows <= 1024 and rows % 64 == 0 and K % 32 == 0 and rows % K == 0, name
        assert c["xp"].shape == (rows, PC.H0) and c["wp"].shape == (PC.H1, PC.H0) and c["xp"].dtype == c["wp"].dtype == torch.int32, name
        assert c["g1"].shape == (rows // K, PC.H1) and c["want"].shape == (rows, PC.H1) and c["want"].dtype == torch.float64, name
        assert torch.isfinite(c["want"]).all(), name
        assert c["bound"] == 1.001 * PC.row_ln_bound(c["gamma"], c["beta"]) + 1e-30
        # the a-priori bound holds for the reference (GELU only shrinks magnitudes)
        assert float(c["want"].abs().max()) <= c["bound"], name
        assert PC.build(name) is c      # built once


def test_plain_bound_stays_below_32():
    """The scale test moves the bound across 32 = 2^5 from below: the cases it runs on must allow any bound from nextafter(32, 0) up."""
    for name, (_, _, kind) in PC.CASES.items():
        if kind == "plain":
            assert PC.build(name)["bound"] < 30.0, name
    assert PC.trip_case(1)["bound"] < 30.0


def test_variance_near_eps():
    c = PC.build("variance near eps")
    assert not c["g1"].any()
    assert bool((c["var"] >= PC.EPS / 4).all()) and bool((c["var"] <= 4 * PC.EPS).all()), (float(c["var"].min()), float(c["var"].max()))


def test_variance_near_eps_can_see_eps():
    """Without eps the result moves by more than 10 % of its magnitude."""
    c = PC.build("variance near eps")
    no_eps, _ = PC.reference(c["xp"], c["sx"], c["wp"], c["sw"], c["g1"], c["rowgroup"], c["gamma"], c["beta"], eps=0.0)
    assert float((no_eps - c["want"]).abs().max()) > 0.1 * float(c["want"].abs().max())
    # and not through a few elements only: the mean change against the mean magnitude
    assert float((no_eps - c["want"]).abs().mean()) > 0.1 * float(c["want"].abs().mean())


def test_row_magnitudes():
    c = PC.build("row magnitudes")
    rmax = c["x"].double().abs().amax(dim=1)
    assert float(rmax.min()) <= 2.0 ** -60 and float(rmax.max()) >= 2.0 ** 40
    assert torch.isfinite(c["want"]).all()
    assert float((c["var"] * PC.H1).max()) < 2.0 ** 120      # the sum of centred squares: fp32 statistics cannot overflow
    # shuffled: every 64-row block mixes rows more than 2^50 apart
    e = torch.log2(rmax).view(-1, 64)
    assert bool(((e.amax(dim=1) - e.amin(dim=1)) > 50).all())
    assert float(c["g1"].abs().max()) > 1.0      # ordinary bias rows
    # the packing keeps the tiny rows (their scales are far from the clamp at 2^-112): the decoded maxima are the inputs' to the hi + lo split's 2^-22
    dmax = unpack_g8(c["xp"], c["sx"], PC.H0).abs().amax(dim=1)
    assert bool(((dmax - rmax).abs() <= 2.0 ** -22 * rmax).all())


def test_rowgroups_96_and_160_change_the_bias_row_at_an_odd_tile():
    for name in ("rowgroup 96", "rowgroup 160"):
        rows, G, _ = PC.CASES[name]
        odd = [b for b in range(G, rows, G) if (b // 32) % 2 == 1]      # group boundaries in the middle of a 64-row block
        assert odd, name
        c = PC.build(name)
        for b in odd:      # and the bias rows on its two sides differ
            assert not torch.equal(c["g1"][b // G - 1], c["g1"][b // G]), (name, b)
    for name, (rows, G, _) in PC.CASES.items():
        if name.startswith("rowgroup"):
            lcm = math.lcm(G, 64)
            assert rows == lcm * -(-192 // lcm), name      # the smallest multiple of both with at least three blocks


def test_row_permutation_crosses_tiles_and_halves_and_fixes_no_row():
    c = PC.build("one bias row")
    perm, n = c["perm"], c["rows"]
    assert c["rowgroup"] == n and c["g1"].shape[0] == 1
    i = torch.arange(n)
    assert torch.equal(perm.sort().values, i)
    assert not bool((perm == i).any())
    assert bool((perm // 32 != i // 32).any()) and bool((perm // 64 != i // 64).any())
    assert bool(((perm % 64) // 32 != (i % 64) // 32).any())      # from one half of a block into the other
    # every 64-row block of the permuted input takes rows from more than one block and from both halves
    src = perm.view(-1, 64)
    assert bool(((src // 64).amax(dim=1) != (src // 64).amin(dim=1)).all())
    assert bool((((src % 64) // 32).amax(dim=1) == 1).all()) and bool((((src % 64) // 32).amin(dim=1) == 0).all())


def test_nan_row_packs_to_nans_and_leaves_the_others():
    c = PC.build("one bias row")
    d = PC.with_nan_row(c)
    keep = torch.arange(c["rows"]) != PC.NAN_ROW
    assert torch.equal(d["xp"][keep], c["xp"][keep]) and torch.equal(d["sx"][keep], c["sx"][keep])
    assert float(d["sx"][PC.NAN_ROW]) == 1.0
    assert torch.isnan(unpack_g8(d["xp"], d["sx"], PC.H0)[PC.NAN_ROW]).all()


def test_gamma_outlier_is_the_existing_special_construction():
    c = PC.build("gamma outlier")
    assert not c["x"][:64].any() and not c["g1"][0].any()
    assert float(c["var"][:64].max()) == 0.0
    assert int(c["gamma"].abs().argmax()) == 13 and float(c["gamma"][13].abs()) > 25 * float(c["gamma"].abs().sort().values[-2])
    assert int(c["x"][100].abs().argmax()) == 7


def test_place_pads_with_nans_aligns_and_guards():
    """`place` on the CPU: the views hold the case's bits at the asked leading dimensions, everything around them is NaN or guard, the pointers keep
    the entry's alignment, and guards_intact sees a write one word outside out or out_scale."""
    c = PC.build("rowgroup 96")
    nan = torch.tensor([PC.NAN_WORD], dtype=torch.int32)
    assert torch.isnan(nan.view(torch.float32)).all() and torch.isnan(nan.view(torch.float16)).all()
    d = PC.place(c, ldx=160, ldw=136, ldrb=528, ldo=520, device="cpu")
    for t, ld, want, align in ((d.x, 160, c["xp"], 32), (d.fw.packed, 136, c["wp"], 32), (d.g1, 528, c["g1"], 16), (d.out, 520, None, 32)):
        assert t.stride() == (ld, 1) and t.data_ptr() % align == 0 and t.dtype == torch.float32
        if want is not None:
            assert torch.equal(t.contiguous().view(torch.int32), want.view(torch.int32))
            whole = torch.as_strided(t, (t.shape[0], ld), (ld, 1)).view(torch.int32)
            assert bool((whole[:, t.shape[1]:] == PC.NAN_WORD).all())
    assert d.out.shape == (192, PC.H1) and d.rs.shape == (192,) and PC.guards_intact(d)
    d.out.zero_(); d.rs.zero_()
    assert PC.guards_intact(d)
    for buf, at in ((d.out_buf, PC.GUARD_WORDS - 1), (d.out_buf, PC.GUARD_WORDS + 192 * 520), (d.out_buf, PC.GUARD_WORDS + PC.H1),
                    (d.rs_buf, PC.GUARD_WORDS - 1), (d.rs_buf, PC.GUARD_WORDS + 192)):
        old = int(buf[at]); buf[at] = 0
        assert not PC.guards_intact(d), at
        buf[at] = old
    a = PC.place(c, arena=True, device="cpu")
    words = a.arena.view(torch.int32)
    base = a.arena.data_ptr()
    live = torch.zeros(words.numel(), dtype=torch.bool)
    for t, want in ((a.sx, c["sx"]), (a.g1, c["g1"]), (a.gamma, c["gamma"]), (a.beta, c["beta"]), (a.sw, c["sw"])):
        assert torch.equal(t, want) and t.is_contiguous() and t.data_ptr() % 16 == 0
        lo = (t.data_ptr() - base) // 4
        assert words[lo - 1] == PC.NAN_WORD and words[lo + t.numel()] == PC.NAN_WORD      # one element before, one past
        live[lo:lo + t.numel()] = True
    assert bool((words[~live] == PC.NAN_WORD).all()) and int((~live).sum()) == 4 * 6      # no more than the alignment between two of them
    assert a.fw.scale is a.sw


def test_head_of_a_trip_case_is_its_first_blocks():
    c = PC.trip_case(5)
    h = PC.head(c, 3)
    assert h["rows"] == 192 and torch.equal(h["xp"], c["xp"][:192]) and torch.equal(h["g1"], c["g1"][:3]) and h["wp"] is c["wp"]
