"""Proves the checker of attention_cases.py on the CPU, without a GPU.  For every case of the table and every element type it applies to, an
fp32 emulation of the kernel that serves it -- tile-wise online softmax with the kernel's tile size, exp2 with the scale folded in, P rounded
to the operand type before the PV product, the denominator from the rounded P where the kernel takes it from a ones row (d = 40, 80) and from
the fp32 P otherwise; for f32x every product as hi hi + 2^-11 (hi lo + lo hi), for k_flash_fwd_x2 the pre-scaled re-split query, the running
maximum rounded up to an fp16 value and P split toward zero; the key ranges of a split launch merged in range order -- meets the per-element
bound and the exact rows, and deliberately broken emulations miss the bound at the cases named below on at least a stated share of the
elements.

Floors of the mutants (share of the elements outside the bound), each from the size of the seeded error against the bound:
  mask_drop        late_max: the dropped key is the dominant one, every element moves by tens of per cent: 0.9.  plain, 77 keys: the dropped
                   key holds a median 0.8 % of the mass, an error of ~ 0.005 against a bf16 bound of ~ 0.0035: 0.3 there; f16 (bound ~ 5e-4: inside it where |v_k - O| < 0.1) 0.8, f32x 0.9
  mask_admit       negative: the admitted key (zero K: score 0 against -150) takes all the mass, its V is zero: 0.9; k_flash_fwd_x2
                   re-reads the last key's row instead, which doubles that key's ~ 1 % of the mass: 0.9 at f32x precision.
                   (At plain bf16 an extra 0.8 % in the denominator is inside 2^-8 (|ref| + S): not asserted there.)
  skip_rescale     late_max, on the LAST tile of the walk (on an earlier one the keys left unscaled are buried by the later rises): the keys
                   before it keep a weight e^16 (e^32 at 64 keys per tile) too large and take the mass from the last key: 0.9
  l_only           late_max: O keeps every earlier tile at full weight while l shrinks it, a factor of e^16 or more: 0.9
  no_log2e         plain: a softmax at temperature 1 / 0.69, probabilities off by tens of per cent: 0.8
  ones_next_head   offset_v, d = 40 / 80: the denominator is ~ 100 times too large: 0.9
  merge_skip       plain: a range with 1 / nsplit of the mass is missing, against an f32x bound: 0.9
  merge_unshifted  plain / late_max: the ranges' maxima differ by ~ 1 (plain) or by dozens (late_max): 0.9
  empty_w1         cannot be caught: an empty range's partial is exactly zero.  Asserted EQUAL to the correct emulation
  empty_stale      the empty range's partial holds the workspace's NaN fill: every element is NaN: 0.99
  x_drop           f32x at plain only (the limit in attention_cases.py): an error in O of about the size of the bound: 0.3
  ragged_row       the last query row of every image keeps the sentinel: exactly 1 / Nq of the elements
"""
import pytest
import torch

from tests import attention_cases as ac

CASE_DT = pytest.mark.parametrize("case,dt", ac.CASE_DT, ids=ac.CASE_DT_IDS)
BF16, F16, F32X = ac.BF16, ac.F16, ac.F32X


@CASE_DT
def test_correct_fp32_emulation_meets_the_bound(case, dt):
    P = ac.problem(case.name, dt)
    name = "%s [%s]" % (case.name, ac.DT_NAME[dt])
    worst = ac.check(ac.emulate(P), P, name)
    print("EMU %s %s %.4f" % (ac.DT_NAME[dt], case.name, worst))
    assert worst <= 1.0
    if case.ws == "split":                               # and the unsplit walk of the same case (what a too-small workspace falls back to)
        ac.check(ac.emulate(P, nsplit=1), P, name + " unsplit")


def _starts(*prefixes):
    return lambda c: c.name.startswith(prefixes)


# mutant -> [(applies(case), element types, floor)]
NAMED = {
    "mask_drop": [(_starts("kind_late_max"), ac.ALL3, 0.9), (_starts("inst_"), (BF16,), 0.3), (_starts("inst_"), (F16,), 0.8), (_starts("inst_"), (F32X,), 0.9)],
    "mask_admit": [(_starts("kind_negative"), ac.ALL3, 0.9)],
    "skip_rescale": [(_starts("kind_late_max"), ac.ALL3, 0.9)],
    "l_only": [(_starts("kind_late_max"), ac.ALL3, 0.9)],
    "no_log2e": [(_starts("inst_", "kind_plain"), ac.ALL3, 0.8)],
    "ones_next_head": [(_starts("kind_offset_v_d40", "kind_offset_v_d80"), ac.ALL3, 0.9)],
    "merge_skip": [(lambda c: c.ws == "split" and c.kind == "plain", (F32X,), 0.9)],
    "merge_unshifted": [(lambda c: c.ws == "split" and c.kind in ("plain", "late_max"), (F32X,), 0.9)],
    "empty_stale": [(_starts("split_empty"), (F32X,), 0.99)],
    "x_drop": [(_starts("inst_", "kind_plain"), (F32X,), 0.3)],
    "ragged_row": [(_starts("inst_", "queries_nq33", "queries_nq129"), ac.ALL3, None)],
}
MUTANT_CASES = [(m, c, dt, floor) for c, dt in ac.CASE_DT for m, rules in NAMED.items() for ok, dts, floor in rules if ok(c) and dt in dts]


def test_every_mutant_is_asserted_somewhere():
    assert {m for m, _, _, _ in MUTANT_CASES} | {"empty_w1"} == set(ac.MUTANTS)
    for m in ("mask_drop", "mask_admit", "skip_rescale", "l_only", "no_log2e", "ones_next_head", "ragged_row"):
        assert {dt for mm, _, dt, _ in MUTANT_CASES if mm == m} == set(ac.ALL3), m


@pytest.mark.parametrize("mutant,case,dt,floor", MUTANT_CASES, ids=["%s-%s-%s" % (m, c.name, ac.DT_NAME[dt]) for m, c, dt, _ in MUTANT_CASES])
def test_broken_emulations_miss_the_bound(mutant, case, dt, floor):
    P = ac.problem(case.name, dt)
    share = ac.outside(ac.emulate(P, mutant), P)
    if floor is None:                                    # ragged_row: the unwritten row and nothing else
        assert abs(share - 1.0 / case.Nq) < 1e-9, share
        return
    print("%s %s [%s]: %.3f of the elements outside the bound (floor %.2f)" % (mutant, case.name, ac.DT_NAME[dt], share, floor))
    assert share > floor, (mutant, case.name, share)


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.name.startswith("split_empty")], ids=repr)
def test_an_empty_range_weighted_one_changes_nothing(case):
    """The one mutant of the list no bound can see: the empty range's partial is (O = 0, l = 0), so its weight does not matter."""
    P = ac.problem(case.name, F32X)
    assert torch.equal(ac.emulate(P, "empty_w1"), ac.emulate(P))


# ------------------------------------------------------------------------------------------------------------------ the table itself
def test_table_reaches_every_instantiation_and_split_path():
    for dt in ac.ALL3:
        got = {ac.kernel_of(c.d, dt)[1] for c in ac.CASES if dt in c.dts and c.name.startswith("inst_")}
        want = ({"k_flash_fwd_x<32, 32, 2>", "k_flash_fwd_x<48, 64, 2>", "k_flash_fwd_x<64, 64, 2>", "k_flash_fwd_x<96, 96, 1>",
                 "k_flash_fwd_x<160, 160, 1>", "k_flash_fwd_x2<40, 64, 2>", "k_flash_fwd_x2<80, 64, 1>"} if dt == F32X else
                {"k_flash_fwd<32, 32, 0>", "k_flash_fwd<48, 64, 40>", "k_flash_fwd<48, 64, 0>", "k_flash_fwd<64, 64, 0>", "k_flash_fwd<96, 96, 80>",
                 "k_flash_fwd<96, 96, 0>", "k_flash_fwd<160, 160, 0>"})
        assert got == want, (dt, got ^ want)
    for c in ac.CASES:
        if c.ws == "none":
            continue
        sp, kt = ac.splits(c.B, c.H, c.Nq, c.Nk, c.d), ac.kernel_of(c.d, F32X)[2]
        ntiles = -(-c.Nk // kt)
        tper = -(-ntiles // sp)
        assert sp > 1 and ac.workspace_bytes(c.B, c.H, c.Nq, c.Nk, c.d) > 0, c.name
        assert (c.nsplit(F32X) == sp) == (c.ws == "split")
        if "_empty_" in c.name:
            assert (sp - 1) * tper >= ntiles, (c.name, sp, tper, ntiles)               # the last range holds no tile
        if "_tail_" in c.name:
            assert (sp - 1) * tper < ntiles and c.Nk % kt != 0, c.name                 # the masked tile is the last range's
        if "_cap8_" in c.name:
            assert sp == 8 and -(-512 // (c.B * c.H)) > 8, c.name
    # every case without a workspace argument runs unsplit, whatever the query would say
    assert all(c.nsplit(dt) == 1 for c, dt in ac.CASE_DT if c.ws != "split")


def test_kinds_do_what_their_names_say():
    for d in (40, 160):
        for dt in ac.ALL3:
            P = ac.problem("kind_large_d%d" % d, dt)
            assert bool(P.exact[:, 0].all()) and 0.0 < float(P.exact.double().mean()) < 0.5            # row 0 by construction, few others
            P = ac.problem("keys_d40_nk1", dt)
            assert bool(P.exact.all())
            for kind, key in (("early_max", 0), ("late_max", 96)):
                P = ac.problem("kind_%s_d%d" % (kind, d), dt)
                c = P.case
                Q, K = P.comp("Q", "val"), P.comp("K", "val")
                s = torch.einsum("bqhi,bkhi->bhqk", Q, K) * P.scale
                assert bool((s.argmax(-1) == key).all()), (kind, d, dt)
                if kind == "late_max":                   # the running maximum rises in every 32-key tile
                    tops = torch.stack([s[..., t:t + 32].max(-1).values for t in range(0, c.Nk, 32)], -1)
                    assert bool((tops[..., 1:] > tops[..., :-1]).all())
            P = ac.problem("kind_negative_d%d" % d, dt)
            s = torch.einsum("bqhi,bkhi->bhqk", P.comp("Q", "val"), P.comp("K", "val")) * P.scale
            assert -170 < float(s.min()) and float(s.max()) < -130
            P = ac.problem("kind_uniform_d%d" % d, dt)
            assert bool(((P.ref - P.comp("V", "val").mean(1, keepdim=True).reshape(1, 1, -1)).abs() < 1e-12).all())
