"""The weight families of tests/weight_families.py are fit for use, shown on the CPU before any GPU sees them: on the read sets
that tests/test_gpu_weights.py runs, every family is

  * ADMISSIBLE (not chaotic): the fp32 oracle's logits are finite and within 2.5e-5 of the float64 value of the same function
    (tests/f64_truth.py; reference model/model.py:32-37). 2.5e-5 is a quarter of the project's 1e-4 parity bar, so the
    "4 x the oracle's max" bar of the GPU test stays inside 1e-4. This is a condition on the INPUTS, not a measurement of a kernel.
    Not admissible, and therefore not among the families: the bias shifts on the unscaled shipped weights (the fp32 oracle is
    itself 6.9 away from float64) and the shipped W_hh x 2 (16.8 away);
  * and COVERS THE GUARDS of the gate math (rd_lstm_t32.hpp stages 3, 5, 8, 9; rd_lstm_f32.hpp; rd_common.hpp rd_sigmoid), whose
    thresholds follow from the code: e_g and e_c are capped at 2^64 = exp2(2.885 x) for x > 22.2; exp2(-1.4427 x) overflows for a
    gate below -88.7 and underflows for a gate above +87.3; exp2(2.885 c) underflows for c < -43.7.

Where a cap is TAKEN is not yet where it MATTERS: without it e would only become inf (and inf x rcp(inf) = NaN) once the exp2
argument passes 128, at g or c > 44.4. The +30 shifts put g at 35 and c at 100..300, so `saturated` and `shipped_half_saturated`
need the cap of e_c but not that of e_g; `random_wide` (g up to 100) needs both, and test_random_wide_... asserts that it gets
there. (Checked once on builds with one cap removed each, see tests/test_gpu_weights.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_families as WF                      # noqa: E402
from f64_truth import f64_forward, f64_forward_stats   # noqa: E402

ADMISSIBLE = 2.5e-5
CAP = 64.0 / 2.88539008177792681                  # 22.2: the fminf(., 64) of e_g and e_c
OVER = -128.0 / 1.44269504088896341               # -88.7: exp2 overflow of e_i, e_f, e_o
UNDER = 126.0 / 1.44269504088896341               # +87.3: their underflow
C_UNDER = -126.0 / 2.88539008177792681            # -43.7: underflow of e_c
E_INF = 128.0 / 2.88539008177792681               # 44.4: where e_g and e_c would be inf without their caps


@pytest.fixture(scope="module")
def evaluated():
    """{(family, -l): (oracle max error against float64, oracle logits, float64 logits, stats)}, computed once"""
    from oracle import oracle as O
    O.build()
    out = {}
    for fam in WF.FAMILIES:
        sd = WF.family(fam)
        ora = O.Oracle(sd)
        for max_len in WF.READ_SETS:
            arena, off, lens = WF.read_set(max_len)
            truth, stats = f64_forward_stats(sd, arena, off, lens, max_len)
            lg = ora.forward_packed(arena, off, lens, max_len)
            out[fam, max_len] = (float(np.abs(lg - truth).max()), lg, truth, stats)
    return out


def test_families_are_seeded_and_shaped():
    for fam in WF.FAMILIES:
        a, b = WF.family(fam), WF.family(fam)
        assert list(a) == WF.KEYS
        for k in WF.KEYS:
            assert a[k].dtype == np.float32 and a[k].shape == WF.SHAPES[k] and np.array_equal(a[k], b[k]) and np.isfinite(a[k]).all()
    rnd, sat, ship, half = WF.family("random"), WF.family("saturated"), WF.shipped(), WF.family("shipped_half_saturated")
    moved = np.flatnonzero(sat["rnn.bias_ih_l0"] != rnd["rnn.bias_ih_l0"])
    want = sorted(int(WF.GATE[g] * WF.H + u) for units, d, _ in WF.shift_groups(19) for g in d for u in units)
    assert sorted(moved) == want and len(want) == 4 * (8 + 3 + 3 + 2 + 4)
    assert len(np.flatnonzero(sat["rnn.bias_ih_l0_reverse"] != rnd["rnn.bias_ih_l0_reverse"])) == 4 * 8
    for k in WF.KEYS:
        if k not in ("rnn.bias_ih_l0", "rnn.bias_ih_l0_reverse"):
            assert np.array_equal(sat[k], rnd[k])
            assert np.array_equal(half[k], ship[k] * np.float32(0.5) if k == "rnn.weight_hh_l0" else ship[k])
    assert np.array_equal((half["rnn.bias_ih_l0"] - ship["rnn.bias_ih_l0"] != 0), (sat["rnn.bias_ih_l0"] != rnd["rnn.bias_ih_l0"]))
    z = WF.family("zero")
    assert z["out.bias"].tolist() == [0.25, -0.5] and all(not z[k].any() for k in WF.KEYS if k != "out.bias")


def test_read_sets_straddle_the_tiles_and_chunks():
    for max_len, (n, (lo, hi)) in WF.READ_SETS.items():
        arena, off, lens = WF.read_set(max_len)
        assert len(lens) == n and n % 64 == 0 and n >= 128 and lens.min() == lo and lens.max() > max_len
        steps = np.minimum(lens, max_len)
        assert (steps == 0).any() and (steps < 64).any() and (steps > 64).any() and (steps == max_len).any()
        if max_len > 128:
            assert ((steps > 128) & (steps < max_len)).any()
        assert (arena == ord("N")).any()


def test_stats_function_is_the_same_arithmetic():
    sd = WF.family("saturated")
    arena, off, lens = WF.read_set(100)
    truth, stats = f64_forward_stats(sd, arena, off, lens, 100)
    assert np.array_equal(truth, f64_forward(sd, arena, off, lens, 100))
    assert sorted(stats) == ["c", "f", "g", "i", "o"] and all(lo <= hi for lo, hi in stats.values())
    # the shipped weights stay far inside every guard: that is the gap the families close
    _, ship = f64_forward_stats(WF.shipped(), arena, off, lens, 100)
    assert max(abs(v) for k in "ifgo" for v in ship[k]) < 30 and max(abs(v) for v in ship["c"]) < 5 and ship["g"][1] < CAP


@pytest.mark.parametrize("max_len", sorted(WF.READ_SETS))
@pytest.mark.parametrize("fam", WF.FAMILIES)
def test_admissible(evaluated, fam, max_len):
    err, lg, truth, _ = evaluated[fam, max_len]
    print("%s -l %d: fp32 oracle max error against float64 %.3g, max |logit| %.3g" % (fam, max_len, err, np.abs(truth).max()))
    assert np.isfinite(lg).all() and np.isfinite(truth).all()
    assert err <= ADMISSIBLE, (fam, max_len, err)


@pytest.mark.parametrize("max_len", sorted(WF.READ_SETS))
@pytest.mark.parametrize("fam", ["saturated", "shipped_half_saturated"])
def test_shifted_families_cover_the_guards(evaluated, fam, max_len):
    st = evaluated[fam, max_len][3]
    print(fam, max_len, st)
    assert st["g"][1] > CAP and st["g"][0] < -CAP
    for k in "ifo":
        assert st[k][0] < OVER, (k, st[k])
    assert st["c"][1] > CAP and st["c"][0] < C_UNDER, st["c"]
    assert st["c"][1] > 0.9 * max_len and st["c"][0] < -0.9 * max_len                        # "about 1 per step", either way
    assert st["c"][1] > E_INF                                                                # the cap of e_c is needed


@pytest.mark.parametrize("max_len", sorted(WF.READ_SETS))
def test_random_wide_covers_overflow_and_underflow_of_every_gate(evaluated, max_len):
    st = evaluated["random_wide", max_len][3]
    print(max_len, st)
    for k in "ifgo":
        assert st[k][1] > UNDER and st[k][0] < OVER, (k, st[k])
    assert st["c"][1] > CAP, st["c"]
    assert st["g"][1] > E_INF and st["c"][1] > E_INF          # both caps are needed, not only taken


def test_zero_family_is_the_bias(evaluated):
    for max_len in WF.READ_SETS:
        err, lg, truth, st = evaluated["zero", max_len]
        assert err == 0.0 and (lg == np.array([0.25, -0.5], dtype=np.float32)).all() and st["c"] == (0.0, 0.0)
