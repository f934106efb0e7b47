"""The recurrence kernels on weights other than the shipped checkpoint (tests/weight_families.py; reference model/model.py:16-37,
whose load_state_dict accepts any weights). tests/test_weight_families_host.py shows on the CPU that every family is admissible
(the fp32 oracle stays within 2.5e-5 of float64) and that the families reach the gate-math guards the shipped weights never reach:
the exp2 argument caps of e_g and e_c, the (1 + e_i)(1 + e_g) and (1 + e_o)(1 + e_c) products that overflow to inf, exp2 overflow
and underflow of every gate, |c| up to 300 - in the classifying kernels, the prefix-state table's rows, tile 1's stashed start
state, the float64 refine pass and the reverse table of the padded semantics.

That the module can fail was checked once on scratch builds with one guard removed each: without the fminf(., 64) of stage 3
(e_g) in rd_lstm_t32.hpp the default kernel's logits are finite but up to 0.94 off on `random_wide` (tests a and e fail; `saturated`
passes, its g stays below the 44.4 where e_g would be inf); without that of stage 8 (e_c), and without the two caps of
rd_lstm_f32.hpp, tests a, c, d, e and f fail on `saturated`, `shipped_half_saturated` and `random_wide` for the kernel concerned.

Yardsticks: the float64 evaluation of tests/f64_truth.py and the CPU oracle with the same weights. Each model is built here
(SeqModel + load_state_dict, as in tests/test_gpu_prefix.py); the session's gpu_model is not touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_families as WF                      # noqa: E402
from f64_truth import f64_forward                 # noqa: E402

pytestmark = pytest.mark.gpu
VARIANTS = ["auto", "mfma_f32", "simple"]
FAMS = ["random", "random_wide", "saturated", "shipped_half_saturated"]
SHIPPED_MAX_LOGIT = 8.7       # the shipped model's largest |logit| on these reads: what the additive slacks of the bars were sized for


@pytest.fixture(scope="module")
def sets():
    """{-l: (arena, off, lens, device batch)} - the read sets of tests/test_weight_families_host.py"""
    from ribodetector_amd.data_loader import seq_encoder as E
    out = {}
    for max_len in WF.READ_SETS:
        arena, off, lens = WF.read_set(max_len)
        out[max_len] = (arena, off, lens, E.batch_from_numpy(arena, off[:-1], lens, "cuda:0"))
    return out


@pytest.fixture(scope="module")
def refs(sets):
    """refs(family) -> (state dict, Oracle, {-l: float64 logits}, {-l: fp32 oracle logits, packed}); computed once per family"""
    from oracle import oracle as O
    O.build()
    cache = {}

    def get(fam):
        if fam not in cache:
            sd = WF.family(fam)
            ora = O.Oracle(sd)
            truth = {L: f64_forward(sd, a, off, lens, L) for L, (a, off, lens, _) in sets.items()}
            packed = {L: ora.forward_packed(a, off, lens, L) for L, (a, off, lens, _) in sets.items()}
            cache[fam] = (sd, ora, truth, packed)
        return cache[fam]
    return get


def _new_model(sd):
    from ribodetector_amd.model import model as M
    m = M.SeqModel(4, 128, 1, 2)
    m.load_state_dict(sd)
    m.set_prefix_table(0)
    m.set_refine(0.0)
    return m.to("cuda:0").eval()


@pytest.fixture(scope="module")
def models(refs):
    """models(family) -> the family's SeqModel on the device (one per family for the whole module, destroyed afterwards); handed
    out in its base state: kernel auto, packed semantics, no refine pass, no prefix table"""
    cache = {}

    def get(fam):
        if fam not in cache:
            cache[fam] = _new_model(refs(fam)[0])
        m = cache[fam]
        m.set_variant("auto")
        m.set_semantics("packed")
        m.set_refine(0.0)
        m.set_prefix_table(0)
        return m
    yield get
    torch.cuda.synchronize()
    for m in cache.values():
        m._destroy()


def _classify(m, b, max_len):
    lg, lab = m.classify_bytes(b.arena, b.offsets, b.lens, max_len)
    torch.cuda.synchronize()
    return lg.clone(), lab.clone()


def _stats(e):
    return {"median": float(np.median(e)), "p99": float(np.quantile(e, 0.99)), "max": float(e.max())}


# ---- a. error against float64, against the reference's own error ----------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMS)
def test_error_against_float64_is_the_oracles(models, refs, sets, report, fam):
    """Every kernel, packed semantics, no refine pass, no table: finite logits, and as close to the float64 value as the fp32 oracle
    is - the bars of test_gpu_parity.test_error_against_float64_truth, their additive slack scaled by s = min(1, max|truth| / 8.7)
    (it was sized for the shipped model's logits and must shrink with the family's); labels equal the float64 labels wherever the
    float64 margin exceeds 2 ek + 2e-4 s."""
    m = models(fam)
    _, _, truth, packed = refs(fam)
    out = report.setdefault("weight_families", {}).setdefault(fam, {})
    failures = []
    for max_len, (arena, off, lens, b) in sets.items():
        tr = truth[max_len]
        s = min(1.0, float(np.abs(tr).max()) / SHIPPED_MAX_LOGIT)
        eo = np.abs(packed[max_len].astype(np.float64) - tr).max(axis=1)
        out["oracle_fp32@%d" % max_len] = dict(_stats(eo), max_abs_logit=float(np.abs(tr).max()))
        for v in VARIANTS:
            m.set_variant(v)
            lg, lab = _classify(m, b, max_len)
            lg, lab = lg.cpu().numpy(), lab.cpu().numpy()
            assert np.isfinite(lg).all(), (fam, v, max_len, "non-finite logits at reads", np.flatnonzero(~np.isfinite(lg).all(axis=1))[:10])
            ek = np.abs(lg.astype(np.float64) - tr).max(axis=1)
            st = _stats(ek)
            st["ratio_to_oracle"] = {k: st[k] / max(out["oracle_fp32@%d" % max_len][k], 1e-30) for k in ("median", "p99", "max")}
            out["%s@%d" % (v, max_len)] = st
            print("%s %s -l %d (s = %.3f): kernel median %.3g p99 %.3g max %.3g | oracle median %.3g p99 %.3g max %.3g"
                  % (fam, v, max_len, s, st["median"], st["p99"], st["max"], np.median(eo), np.quantile(eo, 0.99), eo.max()))
            if not np.median(ek) < 1.5 * np.median(eo) + 2e-7 * s:
                failures.append((v, max_len, "median", st["median"], float(np.median(eo))))
            if not np.quantile(ek, 0.99) < 2.0 * np.quantile(eo, 0.99) + 1e-6 * s:
                failures.append((v, max_len, "p99", st["p99"], float(np.quantile(eo, 0.99))))
            if not ek.max() < 4.0 * eo.max() + 2e-5 * s:
                failures.append((v, max_len, "max", st["max"], float(eo.max())))
            margin = np.abs(tr[:, 1] - tr[:, 0])
            bad = np.flatnonzero(lab != (tr[:, 1] > tr[:, 0]).astype(np.uint8))
            assert (margin[bad] <= 2 * ek[bad] + 2e-4 * s).all(), (fam, v, max_len, "label differs from float64 at margins", margin[bad])
            assert ((lg[:, 1] > lg[:, 0]).astype(np.uint8) == lab).all()
    assert not failures, (fam, failures)


# ---- b. zero weights ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", ["packed", "padded"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_zero_weights_return_the_bias_exactly(models, sets, variant, sem):
    """exp2(0) = 1 in every gate: sigmoid = 1/2 and tanh = 0 exactly, so c = h = 0 and the logits ARE out.bias, bit for bit"""
    m = models("zero")
    m.set_variant(variant)
    m.set_semantics(sem)
    want = torch.tensor([0.25, -0.5], dtype=torch.float32, device="cuda:0")
    for max_len, (_, _, lens, b) in sets.items():
        lg, lab = _classify(m, b, max_len)
        assert torch.equal(lg, want.expand(len(lens), 2)), (variant, sem, max_len, lg[(lg != want).any(1)][:5])
        assert not lab.any()


# ---- c. prefix table: the rows hold saturated state ---------------------------------------------------------------------------

def _steps_and_rows(arena, off, lens, max_len, k, sem):
    """what rd_steps_kernel decides (rd_sort.hpp): remaining steps per read, and whether the read starts from a table row"""
    code_ok = np.zeros(256, dtype=bool)
    code_ok[list(b"ACGTU")] = True
    n = len(lens)
    steps, row = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for i in range(n):
        lr = min(int(lens[i]), max_len)
        T = lr
        if sem == "padded":
            pos = lr - 1
            while pos >= 0 and not code_ok[arena[off[i] + pos]]:
                pos -= 1
            T = pos + 1 if pos >= 0 else max_len
        if T > k and lr >= k and code_ok[arena[off[i]:off[i] + k]].all():
            row[i], T = True, T - k
        steps[i] = T
    return steps, row


def _tiles_surely_holding_a_row(steps, row):
    """The classifying kernels take the reads in order of their remaining steps, longest first; the order INSIDE a bucket of equal
    steps is left to atomics. Tile t holds sorted positions [32 t, 32 t + 32): every read in it has a step count the tile's
    positions span, so if fewer than 32 reads with such a step count start from the zero state, the tile holds a table-started
    read whatever the atomics did. Returns that (sufficient) condition per full tile."""
    srt = np.sort(steps)[::-1]
    sure = []
    for t in range(len(steps) // 32):
        hi, lo = srt[32 * t], srt[32 * t + 31]
        sure.append(int(((steps >= lo) & (steps <= hi) & ~row).sum()) < 32)
    return np.array(sure)


@pytest.mark.parametrize("sem", ["packed", "padded"])
@pytest.mark.parametrize("variant", ["auto", "mfma_f32"])
@pytest.mark.parametrize("fam", ["saturated", "random_wide"])
def test_table_start_from_saturated_rows_is_bit_identical(models, sets, fam, variant, sem):
    """starting a read from its row = stepping over the bases, to the bit (tests/test_gpu_prefix.py) - now with rows that hold
    saturated h and |c| far beyond the shipped model's, in tile 0 (loaded straight) and in tile 1 (stashed in LDS over phase A of
    t = 0) of every workgroup"""
    m = models(fam)
    m.set_variant(variant)
    m.set_semantics(sem)
    for max_len, (arena, off, lens, b) in sets.items():
        m.set_prefix_table(0)
        assert m.prefix_k == 0
        ref_lg, ref_lab = _classify(m, b, max_len)
        assert torch.isfinite(ref_lg).all()
        for k in (4, 7):
            steps, row = _steps_and_rows(arena, off, lens, max_len, k, sem)
            sure = _tiles_surely_holding_a_row(steps, row)
            pairs = sure[0::2] & sure[1::2]                  # workgroup w = tiles 2w, 2w + 1
            # (all but the first workgroup: at -l 100 the longest bucket is the reads of >= 100 bases that the table cannot take)
            assert len(pairs) >= 3 and pairs[1:].all(), (fam, sem, max_len, k, pairs)
            m.set_prefix_table(k)
            assert m.prefix_k == k
            lg, lab = _classify(m, b, max_len)
            assert torch.equal(lg, ref_lg), (fam, variant, sem, max_len, k, float((lg - ref_lg).abs().max()))
            assert torch.equal(lab, ref_lab)


# ---- d. float64 refine pass -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", ["saturated", "random_wide"])
def test_refine_pass_gives_float64_on_saturated_gates(models, refs, sets, fam):
    """Every read through rd_refine_kernel: within 1e-6 max(1, max|truth| / 8.7) of float64 (test_refine_matches_float64...'s bar)
    and the float64 label. The band of rd_set_refine is capped at 1.0 and these families' margins are not, so set_refine(1.0)
    covers the reads inside it (the rest must come back untouched), and the rest go through the same kernel by its pair rule: with
    mate logits equal to -logits every pair margin is 0, inside any band."""
    m = models(fam)
    _, _, truth, _ = refs(fam)
    for max_len, (_, _, _, b) in sets.items():
        tr = torch.from_numpy(truth[max_len]).to("cuda:0")
        bar = 1e-6 * max(1.0, float(tr.abs().max()) / SHIPPED_MAX_LOGIT)
        want_lab = (tr[:, 1] > tr[:, 0]).to(torch.uint8)
        m.set_refine(0.0)
        lg0, lab0 = _classify(m, b, max_len)
        m.set_refine(1.0)
        lg1, lab1 = _classify(m, b, max_len)
        band = (lg0[:, 1] - lg0[:, 0]).abs() < 1.0
        assert int(band.sum()) > 0
        assert torch.equal(lg1[~band], lg0[~band]) and torch.equal(lab1[~band], lab0[~band])
        assert float((lg1[band].double() - tr[band]).abs().max()) < bar
        assert torch.equal(lab1[band], want_lab[band])
        m.refine(b.arena, b.offsets, b.lens, max_len, lg0, lab0, mate_logits=(-lg0).contiguous(), thresh=1.0)
        torch.cuda.synchronize()
        err = float((lg0.double() - tr).abs().max())
        print("%s -l %d: refined max error %.3g (bar %.3g)" % (fam, max_len, err, bar))
        assert torch.isfinite(lg0).all() and err < bar, (fam, max_len, err)
        assert torch.equal(lab0, want_lab)
        assert torch.equal(lg0[band], lg1[band])            # one pass, whichever way a read got into it
    m.set_refine(0.0)


# ---- e. padded semantics: rd_revtab_kernel with a reverse recurrent matrix of ordinary size -------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("fam", ["random", "saturated", "random_wide"])
def test_padded_semantics_against_the_oracle(models, refs, sets, report, fam, variant):
    """1e-4 on every logit and labels equal outside a 2e-4 margin (test_gpu_parity._check) against the oracle's restatement of the
    reference's CPU product: the reverse direction runs max_len - 1 - pos steps over zero rows through weight_hh_l0_reverse, which
    is all but zero in the shipped checkpoint (|w| <= 0.088) and of ordinary size (sigma 1/sqrt(128)) here"""
    m = models(fam)
    _, ora, _, _ = refs(fam)
    m.set_variant(variant)
    m.set_semantics("padded")
    out = report.setdefault("weight_families", {}).setdefault(fam, {})
    for which, max_len in ((100, 100), (300, 100), (100, 64)):
        arena, off, lens, b = sets[which]
        ref = ora.forward_padded(arena, off, lens, max_len)
        lg, lab = _classify(m, b, max_len)
        lg, lab = lg.cpu().numpy(), lab.cpu().numpy()
        assert np.isfinite(lg).all() and np.isfinite(ref).all()
        err = float(np.abs(lg - ref).max())
        out["padded_%s_set%d@%d" % (variant, which, max_len)] = err
        print("%s %s padded, set %d at -l %d: max |logit - oracle| %.3g" % (fam, variant, which, max_len, err))
        assert err < 1e-4, (fam, variant, which, max_len, err)
        ref_lab = (ref[:, 1] > ref[:, 0]).astype(np.uint8)
        bad = np.flatnonzero(lab != ref_lab)
        assert (np.abs(ref[:, 1] - ref[:, 0])[bad] < 2e-4).all()
        assert ((lg[:, 1] > lg[:, 0]).astype(np.uint8) == lab).all()
    # the switch is live on these weights too
    arena, off, lens, b = sets[100]
    m.set_semantics("packed")
    assert np.abs(_classify(m, b, 100)[0].cpu().numpy() - ora.forward_padded(arena, off, lens, 100)).max() > 1e-2


# ---- f. load_state_dict on a live model -----------------------------------------------------------------------------------------

def test_reload_on_a_live_model(models, refs, sets):
    """load_state_dict on a model that is on the device re-creates the handle with the new weights (the reference's
    load_state_dict works on a live module too); a prefix-state table attached before is rebuilt for them, never read as the
    new model's rows"""
    _, _, _, b = sets[100]
    want_sat = _classify(models("saturated"), b, 100)
    m = _new_model(refs("random")[0])
    try:
        first = _classify(m, b, 100)
        m.set_prefix_table(5)
        assert m.prefix_k == 5 and torch.equal(_classify(m, b, 100)[0], first[0])
        m.load_state_dict(refs("saturated")[0])
        assert m._handle is not None and m.prefix_k == 5
        with_table = _classify(m, b, 100)
        m.set_prefix_table(0)
        without = _classify(m, b, 100)
        assert torch.equal(with_table[0], without[0]) and torch.equal(with_table[1], without[1])
        assert torch.equal(without[0], want_sat[0]) and not torch.equal(without[0], first[0])
        m.set_prefix_table(5)
        m.load_state_dict(refs("random")[0])
        last = _classify(m, b, 100)
        assert m.prefix_k == 5 and torch.equal(last[0], first[0]) and torch.equal(last[1], first[1])
        # a refused state dict leaves the live model as it was
        bad = {k: v.copy() for k, v in refs("random")[0].items()}
        bad["rnn.weight_hh_l0"][3, 3] = np.inf
        with pytest.raises(RuntimeError, match="non-finite"):
            m.load_state_dict(bad)
        assert torch.equal(_classify(m, b, 100)[0], first[0])
    finally:
        torch.cuda.synchronize()
        m._destroy()
