"""Turbo codes on the CPU: the specification tests/turbo_f32.py against the reference-executed fixture
(tests/golden/turbo_ref_golden.npz, tools/gen_turbo_ref_golden.py), the QPP table, the index tables handed to the kernels of
csrc/turbo.hip (their bounds are checked here, not on the GPU), the constructor refusals, the signatures, the properties and
the import path; and the condition on the bits that tests/test_gpu_turbo.py cannot compare (tests/turbo_cases.py).

The bar of the soft outputs of map / log, measured, not guessed: the reference's own single-precision result against its own
double-precision result on the same inputs, e32 = max |ref32 - ref64| over the 20 codewords of a case, times 4, plus one
float32 ulp at the codeword's largest |LLR|.  e32 is taken over the case and not per codeword: the specification sums over
the states in another order than the reference (halving fold against reduce_sum), so its rounding error on a codeword is
another draw from the same distribution, and the largest of 20 draws estimates that distribution where a single draw does
not (per codeword, two of the 40 case / algorithm pairs exceed 4 times their own codeword's draw, by a factor 1.4).
Measured over the 20 cases of the fixture (3 to 8 iterations):
  map  e32 per case 4.2e-6 .. 5.8e-5
  log  e32 per case 6.4e-5 .. 1.3e-3
and the specification's float32 output uses at most 0.51 of the bar.  (log carries the metrics unnormalised, so its float32
error grows with the length and the LLR sum of the codeword; map normalises at every step.)  The float64 specification lies
within 2e-12 of the reference's double-precision output."""
import json
import os

import numpy as np
import pytest

import turbo_cases as tc
import turbo_f32 as spec
from sionna_amd.phy.fec.interleaving import QPP_COEFFS, Deinterleaver, Turbo3GPPInterleaver, qpp_perm
from sionna_amd.phy.fec.turbo import TurboDecoder, TurboEncoder, TurboTermination, polynomial_selector, puncture_pattern
from sionna_amd.phy.fec.turbo.utils import turbo_tables

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "turbo_ref_golden.npz"))
CASES = [str(c) for c in G["cases"]]
BAR_C = 4.0


def _case(name):
    p = name + "/"
    return (tuple(str(x) for x in G[p + "gen_poly"]), 1 / int(G[p + "rate_inv"]), bool(G[p + "terminate"]), int(G[p + "num_iter"]),
            G[p + "perm"], p)


def test_the_fixture_covers_the_issue_s_cases():
    assert len(CASES) == 20
    seen = {(int(G[c + "/rate_inv"]), bool(G[c + "/terminate"]), len(str(G[c + "/gen_poly"][0]))) for c in CASES}
    assert seen >= {(r, t, K) for r in (2, 3) for t in (False, True) for K in (3, 4, 5, 6)}
    assert sum("rand" in c for c in CASES) == 2 and any(c + "/map_hard" in G for c in CASES)
    for c in CASES:
        assert G[c + "/u"].shape[0] == 20 and G[c + "/u"].shape[1] <= 128


@pytest.mark.parametrize("name", CASES)
def test_encoder_spec_bit_exact(name):
    gp, rate, term, _, perm, p = _case(name)
    assert np.array_equal(spec.encode(G[p + "u"], gp, perm, rate, term), G[p + "c"])


@pytest.mark.parametrize("name", CASES)
def test_maxlog_spec_bit_exact(name):
    gp, rate, term, it, perm, p = _case(name)
    got = spec.decode(G[p + "llr"], gp, perm, rate, term, it, False, "maxlog")
    assert got.dtype == np.float32 and np.array_equal(got, G[p + "maxlog_single"])
    if p + "maxlog_hard" in G:
        assert np.array_equal(spec.decode(G[p + "llr"], gp, perm, rate, term, it, True, "maxlog"), G[p + "maxlog_hard"])
    if p + "maxlog_double" in G:
        got = spec.decode(G[p + "llr"], gp, perm, rate, term, it, False, "maxlog", dtype=np.float64)
        assert got.dtype == np.float64 and np.array_equal(got, G[p + "maxlog_double"])


@pytest.mark.parametrize("alg", ["map", "log"])
@pytest.mark.parametrize("name", CASES)
def test_soft_spec_against_reference(name, alg):
    """|spec32 - ref64| <= 4 e32 + ulp32(max |ref64| of the codeword), e32 = max |ref32 - ref64| over the case; the hard
    decisions wherever the reference's |LLR| exceeds that bar"""
    gp, rate, term, it, perm, p = _case(name)
    r32, r64 = G[p + f"{alg}_single"].astype(np.float64), G[p + f"{alg}_double"]
    e32 = np.max(np.abs(r32 - r64))
    bar = BAR_C * e32 + np.spacing(np.max(np.abs(r64), axis=-1).astype(np.float32)).astype(np.float64)
    got = spec.decode(G[p + "llr"], gp, perm, rate, term, it, False, alg)
    d = np.max(np.abs(got.astype(np.float64) - r64), axis=-1)
    print(f"{name} {alg}: e32 {e32:.3e}, spec32 - ref64 {d.max():.3e}, largest share of the bar {np.max(d / bar):.2f}")
    assert got.dtype == np.float32 and np.all(d <= bar), (name, alg, d.max(), bar.min())
    if p + f"{alg}_hard" in G:
        hard = spec.decode(G[p + "llr"], gp, perm, rate, term, it, True, alg)
        sure = np.abs(r64) > bar[:, None]
        assert sure.mean() > 0.99 and np.array_equal(hard[sure], G[p + f"{alg}_hard"][sure])


# ---------------------------------------------------------------- interleaver
@pytest.mark.parametrize("K", [40, 41, 48, 512, 1000, 6144])
def test_qpp_permutation_matches_the_reference(K):
    il = Turbo3GPPInterleaver()
    assert np.array_equal(il._generate_perm_full(K), G[f"qpp/perm_{K}"])
    assert np.array_equal(il._generate_perm_full(K, inverse=True), G[f"qpp/inv_{K}"])
    assert np.array_equal(qpp_perm(K), G[f"qpp/perm_{K}"])


def test_qpp_table_rows_are_permutations():
    assert len(QPP_COEFFS) == 188 == int(G["qpp/num_rows"])
    for K, (f1, f2) in QPP_COEFFS.items():
        i = np.arange(K, dtype=np.int64)
        assert np.array_equal(np.sort((f1 * i + f2 * i * i) % K), i), K
    for K, f1, f2 in G["qpp/coeff_rows"]:
        assert QPP_COEFFS[int(K)] == (int(f1), int(f2))
    assert sorted(int(r[0]) for r in G["qpp/coeff_rows"]) == [40, 48, 512, 1008, 6144]


def test_qpp_pruning_and_refusal():
    full, pruned = qpp_perm(1008), qpp_perm(1000)
    assert np.array_equal(pruned, full[full < 1000]) and np.array_equal(np.sort(pruned), np.arange(1000))
    with pytest.raises(ValueError):
        qpp_perm(6145)
    with pytest.raises(ValueError):
        Turbo3GPPInterleaver().build((2, 6145))
    with pytest.raises(ValueError):
        Turbo3GPPInterleaver(axis=2).build((2, 40))
    with pytest.raises(TypeError):
        Turbo3GPPInterleaver(axis=1.0)
    with pytest.raises(TypeError):
        Turbo3GPPInterleaver(inverse=1)
    assert Deinterleaver(Turbo3GPPInterleaver()).interleaver.axis == -1


# ---------------------------------------------------------------- index tables: the bound check of the kernels
SIZES = sorted(set(QPP_COEFFS) | {1, 2, 3, 41, 43, 1000, 6143})


@pytest.mark.parametrize("terminate", [False, True])
@pytest.mark.parametrize("rate", [1/3, 1/2])
def test_index_tables_stay_inside_the_codeword(rate, terminate):
    """every table handed to samd_turbo_encode / samd_turbo_bcjr lies in [-1, n); perm / inv are inverse permutations; the
    positions an encoder writes (with the padding) are exactly 0..n-1, each once; every constraint length"""
    for mu in (2, 3, 4, 5, 7):
        for k in SIZES if mu == 3 else SIZES[::17] + [41, 43]:
            t = turbo_tables(k, rate, terminate, mu, qpp_perm(k))
            n, T = t["n"], t["T"]
            assert T == k + (mu if terminate else 0)
            rows = k + (-(-4 * mu // 3) if terminate else 0)
            assert n == (3 * rows if rate == 1/3 else 2 * rows)
            for name, shape in (("idx1", (T, 2)), ("idx2", (T, 2)), ("opos", (2, T, 2)), ("zpos", (2,))):
                a = t[name]
                assert a.dtype == np.int32 and a.shape == shape and a.flags.c_contiguous, name
                assert a.min() >= -1 and a.max() < n, (name, k, mu)
            for name in ("perm", "inv"):
                assert t[name].dtype == np.int32 and np.array_equal(np.sort(t[name]), np.arange(k)), name
            assert np.array_equal(t["perm"][t["inv"]], np.arange(k)) and np.array_equal(t["inv"][t["perm"]], np.arange(k))
            written = np.concatenate([t["opos"].ravel(), t["zpos"]])
            written = written[written >= 0]
            assert np.array_equal(np.sort(written), np.arange(n)), (k, mu)
            assert np.array_equal(t["idx1"][:k, 0], t["idx2"][t["inv"], 0])    # decoder 2 reads decoder 1's systematic values interleaved
            assert (t["idx1"][:k, 0] >= 0).all()                              # no systematic information bit is punctured


def test_index_tables_agree_with_the_specification():
    """reading a codeword through idx1 / idx2 gives the y1_cw / y2_cw that turbo_f32.split assembles"""
    rng = np.random.default_rng(5)
    for rate in (1/3, 1/2):
        for terminate in (False, True):
            for k, mu in ((40, 2), (41, 3), (43, 3), (64, 4), (45, 5)):
                gp = polynomial_selector(mu + 1)
                perm = qpp_perm(k)
                t = turbo_tables(k, rate, terminate, mu, perm)
                y = rng.normal(size=(2, t["n"])).astype(np.float32)
                k2, y1, y2 = spec.split(y, gp, perm, rate, terminate)
                assert k2 == k
                ypad = np.concatenate([y, np.zeros((2, 1), np.float32)], axis=1)          # index -1 reads 0
                assert np.array_equal(ypad[:, t["idx1"].ravel()], y1) and np.array_equal(ypad[:, t["idx2"].ravel()], y2)
    with pytest.raises(ValueError):
        turbo_tables(4, 1/3, False, 2, [0, 1, 1, 2])


# ---------------------------------------------------------------- termination, pattern, selector
@pytest.mark.parametrize("K", [3, 4, 5, 6])
def test_termination_round_trip(K):
    p = f"term/K{K}/"
    tt = TurboTermination(K)
    assert tt.get_num_term_syms() == int(G[p + "num_syms"])
    merged = tt.termbits_conv2turbo(G[p + "t1"], G[p + "t2"])
    assert np.array_equal(merged, G[p + "merged"])
    b1, b2 = tt.term_bits_turbo2conv(merged)
    assert np.array_equal(b1, G[p + "back1"]) and np.array_equal(b2, G[p + "back2"])
    assert np.array_equal(b1, G[p + "t1"]) and np.array_equal(b2, G[p + "t2"])


def test_polynomial_selector_and_pattern():
    assert [polynomial_selector(K) for K in (3, 4, 5, 6)] == [('111', '101'), ('1011', '1101'), ('10011', '11011'), ('111101', '101011')]
    assert puncture_pattern(1/2, 1/2).tolist() == [[True, True, False], [True, False, True]]
    assert puncture_pattern(1/3, 1/2).tolist() == [[True, True, True]]


def test_polynomial_selector_refuses_a_float():
    with pytest.raises(TypeError):
        polynomial_selector(4.0)


@pytest.mark.parametrize("K", [2, 7])
def test_polynomial_selector_refuses_the_length(K):
    with pytest.raises(ValueError):
        polynomial_selector(K)


def test_puncture_pattern_refuses_other_rates():
    with pytest.raises(NotImplementedError):
        puncture_pattern(1/4, 1/2)
    with pytest.raises(ValueError):
        puncture_pattern(1/3, 1/3)


def test_termination_refuses_more_than_two_encoders():
    with pytest.raises(NotImplementedError):
        TurboTermination(4, num_conv_encs=3)


# ---------------------------------------------------------------- constructor refusals (encoding.py:108-131, decoding.py:125-168)
@pytest.mark.parametrize("cls", [TurboEncoder, TurboDecoder])
def test_refuses_gen_poly_that_is_not_strings(cls):
    with pytest.raises(TypeError):
        cls(gen_poly=(1011, 1101))


@pytest.mark.parametrize("cls", [TurboEncoder, TurboDecoder])
def test_refuses_gen_poly_of_unequal_lengths(cls):
    with pytest.raises(ValueError):
        cls(gen_poly=("1011", "110"))


@pytest.mark.parametrize("cls", [TurboEncoder, TurboDecoder])
def test_refuses_gen_poly_with_other_characters(cls):
    with pytest.raises(ValueError):
        cls(gen_poly=("1021", "1101"))


def test_encoder_refuses_three_polynomials():
    with pytest.raises(ValueError):
        TurboEncoder(gen_poly=("1011", "1101", "1111"))


def test_decoder_refuses_three_polynomials():
    with pytest.raises(ValueError):                                 # puncture_pattern's check of the constituent rate
        TurboDecoder(gen_poly=("1011", "1101", "1111"))


@pytest.mark.parametrize("cls", [TurboEncoder, TurboDecoder])
@pytest.mark.parametrize("K", [2, 7, None])
def test_refuses_the_constraint_length(cls, K):
    with pytest.raises(ValueError):
        cls(constraint_length=K)


@pytest.mark.parametrize("cls", [TurboEncoder, TurboDecoder])
def test_refuses_the_rate(cls):
    with pytest.raises(ValueError):
        cls(constraint_length=4, rate=1/4)


@pytest.mark.parametrize("cls", [TurboEncoder, TurboDecoder])
def test_refuses_terminate_that_is_not_bool(cls):
    with pytest.raises(TypeError):
        cls(constraint_length=4, terminate=1)


def test_refuses_the_interleaver():
    with pytest.raises(ValueError):
        TurboEncoder(constraint_length=4, interleaver_type="qpp")
    with pytest.raises(ValueError):
        TurboDecoder(constraint_length=4, interleaver="Random")


def test_decoder_refuses_hard_out_that_is_not_bool():
    with pytest.raises(TypeError):
        TurboDecoder(constraint_length=4, hard_out=1)


def test_decoder_refuses_the_algorithm():
    with pytest.raises(ValueError):
        TurboDecoder(constraint_length=4, algorithm="max")


@pytest.mark.parametrize("cls", [TurboEncoder, TurboDecoder])
def test_gen_poly_up_to_constraint_length_8(cls):
    assert cls(gen_poly=tc.GEN_POLY_8).constraint_length == 8
    with pytest.raises(ValueError, match="constraint lengths 3..8"):
        cls(gen_poly=("100110111", "111001011"))


def test_build_refusals():
    with pytest.raises(ValueError):
        TurboEncoder(constraint_length=4).build((2, 6145))
    TurboEncoder(constraint_length=4, interleaver_type="random").build((2, 6145))
    with pytest.raises(ValueError):
        TurboDecoder(constraint_length=4, rate=1/2).build((2, 81))          # odd n at rate 1/2
    with pytest.raises(ValueError):
        TurboDecoder(constraint_length=4, terminate=True).build((2, 133))   # 133 - 12 termination bits: not a multiple of 3
    with pytest.raises(ValueError):
        TurboDecoder(constraint_length=4, terminate=True).build((2, 9))     # shorter than the termination


def test_properties_before_and_after_build():
    enc = TurboEncoder(constraint_length=4, rate=1/3, terminate=True)
    assert enc.gen_poly == ("1011", "1101") and enc.constraint_length == 4 and enc.terminate and enc.k is None and enc.n is None
    assert enc.coderate == 1/3 and enc.punct_pattern.tolist() == [[True, True, True]] and enc.trellis.rsc
    enc.build((5, 40))
    assert enc.k == 40 and enc.n == 120 and abs(enc.coderate - 40 / 132) < 1e-15
    dec = TurboDecoder(enc, num_iter=3)
    assert dec.k is None and dec.n is None and dec.coderate == 1/3 and dec.trellis is enc.trellis and dec.gen_poly == enc.gen_poly
    assert dec.internal_interleaver is enc.internal_interleaver and dec.constraint_length == 4 and dec.num_iter == 3
    dec.build((5, 132))
    assert dec.k == 40 and dec.n == 132
    dec = TurboDecoder(constraint_length=5, rate=1/2, terminate=False, interleaver="random")
    dec.build((2, 3, 90))
    assert dec.k == 45 and dec.n == 90 and dec.coderate == 1/2
    enc = TurboEncoder(constraint_length=3, rate=1/2)
    enc.build((40,))
    assert enc.k == 40 and enc.n == 80 and enc.coderate == 1/2
    assert TurboEncoder(precision="double").precision == "double" and TurboDecoder(constraint_length=3, precision="double").precision == "double"


def test_signatures_match_the_reference():
    from test_api_signatures import _check
    with open(os.path.join(GOLD, "turbo_api_signatures.json")) as f:
        sig = json.load(f)["signatures"]
    assert set(sig) == {"fec.turbo.polynomial_selector", "fec.turbo.puncture_pattern", "fec.turbo.TurboTermination",
                        "fec.turbo.TurboEncoder", "fec.turbo.TurboDecoder", "fec.interleaving.Turbo3GPPInterleaver"}
    import sionna_amd.phy.fec.interleaving as interleaving
    import sionna_amd.phy.fec.turbo as turbo
    for name, ref in sig.items():
        obj = getattr(interleaving if "interleaving" in name else turbo, name.rsplit(".", 1)[1])
        if ref["kind"] == "function":
            _check(ref["params"], obj, name)
            continue
        _check(ref["__init__"], obj.__init__, name + ".__init__")
        if ref.get("call"):
            _check(ref["call"], obj.call, name + ".call")
        for attr, kind, _ in ref["public"]:
            assert hasattr(obj, attr), (name, attr)


def test_import_path_under_install_as_sionna():
    import sionna_amd
    sionna_amd.install_as_sionna(tf_shim=True)
    from sionna.phy.fec.turbo import TurboDecoder as D, TurboEncoder as E
    from sionna.phy.fec.interleaving import Turbo3GPPInterleaver as I
    import sionna.phy.fec as fec
    assert (D, E, I) == (TurboDecoder, TurboEncoder, Turbo3GPPInterleaver) and fec.turbo.TurboTermination is TurboTermination


# ---------------------------------------------------------------- the condition of the GPU test's hard-decision comparison
@pytest.mark.parametrize("cid,alg", tc.SOFT_PAIRS)
def test_few_bits_are_below_the_anchored_bar(cid, alg):
    """spec32 against spec64 alone: at the m of the case at most 1 % of the bits have |spec64 LLR| within the anchored bar
    (tests/test_gpu_turbo.py compares the hard decisions of the others), and spec32 itself decides those like spec64"""
    r32, r64 = tc.refs(cid, alg)
    bar, sure = tc.bar_and_mask(cid, alg)
    print(f"{cid} {alg}: bar max {bar.max():.3e}, bits below it {1 - sure.mean():.4f}")
    assert np.isfinite(r32).all() and np.isfinite(r64).all()
    assert 1 - sure.mean() <= tc.MAX_SKIPPED
    assert np.array_equal((r32 > 0)[sure], (r64 > 0)[sure])
