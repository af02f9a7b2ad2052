"""Lift, centered bits and noise measurement on the MI355X (the HIP build): the cases of tests/test_noise_emu.py on
every stock set of tests/ref_params.py with the FP64 kernels on and off (the inverse transform of the phase takes
different instances), on C2 (4 x 60 bits), on rows larger than one LDS tile, on an N = 32768, L = 16 shape and on
batches that are not a multiple of anything; the kernel symbols the profiler saw name the intended L instances."""
import random
import re

import numpy as np
import pytest

import devop_cases as D
import devop_shapes as S
import encode_cases as E
import noise_cases as N
import ref_params
from helpers import HIP_LIB, Xfer, load_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


def instances(fhe, fn):
    """{(L, bits)}: the lift_kernel instances launched while fn() ran, from the profiler's kernel symbols."""
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        fn()
        symbols = [sym for _label, sym, _n, _ms in fhe.prof_entries()]
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    found = [re.search(r"lift_kernel<(\d+), (true|false)>", s) for s in symbols]
    return {(int(m.group(1)), m.group(2) == "true") for m in found if m}


def stock(fhe, n):
    return E.params(fhe, n, ref_params.plaintext_modulus(n), moduli=ref_params.DEFAULT_128[n])


def test_lift_every_set(fhe):
    """L = 1, 2, 3, 4, 5, 9, 16; 36 ... 62-bit moduli; bitlen(q) below, on and above a multiple of 64; N = 1024 (four
    workgroups per polynomial).  Then every other compile-time L (6, 7, 8, 10 ... 15) at N = 256."""
    sets = N.lift_sets(1024)
    seen = instances(fhe, lambda: [N.case_lift(fhe, True, 1024, m, columns=range(0, 1024, 7)) for m in sets])
    assert seen == {(L, False) for L in (1, 2, 3, 4, 5, 9, 16)}, seen
    seen = instances(fhe, lambda: [N.case_centered_bits(fhe, True, 1024, m) for m in sets])
    assert seen == {(L, True) for L in (1, 2, 3, 4, 5, 9, 16)}, seen
    # the remaining compile-time instances (L = 6, 7, 8, 10 ... 15) at N = 256: with the sets above, every L = 1 ... 16
    more = N.lift_more_sets()
    rest = (6, 7, 8, 10, 11, 12, 13, 14, 15)
    seen = instances(fhe, lambda: [N.case_lift(fhe, True, N.LIFT_MORE_N, m) for m in more])
    assert seen == {(L, False) for L in rest}, seen
    seen = instances(fhe, lambda: [N.case_centered_bits(fhe, True, N.LIFT_MORE_N, m) for m in more])
    assert seen == {(L, True) for L in rest}, seen
    assert {L for L in rest} | {1, 2, 3, 4, 5, 9, 16} == set(range(1, 17))


def test_generic_instance(fhe):
    m = N.generate_moduli([40] * 17, 2048)
    seen = instances(fhe, lambda: (N.case_lift(fhe, True, 2048, m, batch=1, columns=range(0, 2048, 5)),
                                   N.case_centered_bits(fhe, True, 2048, m)))
    assert seen == {(0, False), (0, True)}, seen


# stock n = 1024 has one 27-bit modulus against t of 20 bits: a fresh public-key ciphertext carries more noise than the
# 6 bits that leaves, so it does not decrypt to its plaintext; everything else is checked there as on the other sets
DECRYPTS = {n: n != 1024 for n in ref_params.DEFAULT_128}


@pytest.mark.parametrize("n", sorted(ref_params.DEFAULT_128))
def test_stock_sets(fhe, n):
    """Lift and centered bits over the set's own moduli, then the noise cases at level 0 and at the deepest level, F64
    on and off (the oracle sees the same ciphertexts both times: every seed is fixed).  n = 1024 and 2048 have one
    modulus: level 0 is the deepest level."""
    opar, par = stock(fhe, n)
    L = len(opar.moduli)
    seen = instances(fhe, lambda: (N.case_lift(fhe, True, n, opar.moduli, batch=1, columns=range(0, n, 97)),
                                   N.case_centered_bits(fhe, True, n, opar.moduli)))
    assert seen == {(L, False), (L, True)}, seen
    one = (lambda b: [b - 1]) if n > 4096 else None
    for f64 in (True, False):
        fhe.set_f64(f64)
        try:
            seen = instances(fhe, lambda: N.case_noise_parity(fhe, True, opar, par, level=0, batch=2, check_items=one))
            assert seen == {(L, True)}, (f64, seen)
            N.case_null_vs_given(fhe, True, opar, par, level=0, batch=1, decrypts=DECRYPTS[n])
            if opar.max_level() > 0:
                seen = instances(fhe, lambda: N.case_noise_parity(fhe, True, opar, par, level=opar.max_level(), batch=2,
                                                                  check_items=one, seed=13))
                assert seen == {(1, True)}, (f64, seen)
        finally:
            fhe.set_f64(True)


def test_c2(fhe):
    """BASELINE's C2: N = 8192, four 60-bit moduli (integer kernels)."""
    n = 8192
    opar, par = E.params(fhe, n, ref_params.plaintext_modulus(n), moduli_sizes=[60] * 4)
    seen = instances(fhe, lambda: N.case_noise_parity(fhe, "abi", opar, par, level=0, batch=2, check_items=lambda b: [0]))
    assert seen == {(4, True)}, seen
    N.case_noise_parity(fhe, True, opar, par, level=1, batch=1, seed=17)
    N.case_null_vs_given(fhe, True, opar, par, level=0, batch=1)


@pytest.mark.parametrize("i", range(3), ids=["general", "class3", "t61"])
def test_null_vs_given(fhe, i):
    opar, par = D.params(fhe, S.roundtrip_shapes()[i])
    N.case_null_vs_given(fhe, True, opar, par, level=0, batch=2)


def test_past_decryption_failure(fhe):
    opar, par = E.params(fhe, 1024, E.stock_t(1024), moduli_sizes=[62, 50])
    N.case_past_decryption_failure(fhe, True, opar, par)
    opar, par = E.params(fhe, 16, 1153, moduli_sizes=[62, 50])
    N.case_past_decryption_failure(fhe, "abi", opar, par)


def test_rows_larger_than_lds(fhe):
    """N = 32768: the phase's inverse transform runs its first stages through global memory."""
    n = 32768
    opar, par = E.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 55, 60])
    N.case_null_vs_given(fhe, "abi", opar, par, level=0, batch=1)


def test_n32768_l16(fhe):
    """C5's chain length: sixteen 60-bit moduli at N = 32768 -- the L = 16 instances, 128 workgroups per polynomial."""
    n = 32768
    m = N.generate_moduli([60] * 16, n)
    seen = instances(fhe, lambda: (N.case_lift(fhe, True, n, m, batch=1, columns=list(range(0, n, 1021)) + [255, 256, n - 1]),
                                   N.case_centered_bits(fhe, True, n, m)))
    assert seen == {(16, False), (16, True)}, seen


@pytest.mark.parametrize("batch", [1, 3, 227, 1024])
def test_batches(fhe, batch):
    """Batches that are not a multiple of anything: every polynomial's centered bits against the formula on the lifted
    integers (N = 512, five moduli: the oracle's lift runs in Python), sampled lifts against the oracle, and the
    noise of a batch of fresh ciphertexts on stock n = 4096, first and last item against the oracle."""
    n = 512
    moduli = N.generate_moduli([52, 51, 51, 51, 51], n)
    x = Xfer(True)
    ctx = fhe.Context(moduli, n)
    g = np.random.default_rng(batch)
    polys = np.stack([np.stack([g.integers(0, m, size=n, dtype=np.uint64) for m in moduli]) for _ in range(batch)])
    # a few polynomials of small centered coefficients, so that the maxima differ across the batch
    q = 1
    for m in moduli:
        q *= m
    rng = random.Random(batch)
    for b in range(0, batch, 5):
        k = rng.randrange(1, q.bit_length() - 1)
        polys[b] = N.residues(moduli, [rng.choice([1, -1]) * rng.randrange(1 << k) % q for _ in range(n)])
    inp = x.to(polys)
    got_bits = [int(v) for v in x.back(ctx.centered_bits(inp))]
    limbs = x.back(ctx.lift(inp)).astype(object)
    ints = sum(limbs[..., k] << (64 * k) for k in range(limbs.shape[-1]))
    assert got_bits == [max(N.cbits(int(v), q) for v in ints[b]) for b in range(batch)]
    from fhe_oracle.rns import RnsContext
    rns = RnsContext(moduli)
    for b in sorted({0, batch // 2, batch - 1}):
        for j in (0, 255, 256, n - 1):
            assert int(ints[b][j]) == rns.lift([int(polys[b][i][j]) for i in range(len(moduli))])
    opar, par = stock(fhe, 4096)
    N.case_null_vs_given(fhe, True, opar, par, level=0, batch=batch, seed=batch) if batch <= 3 else \
        N.case_noise_parity(fhe, True, opar, par, level=0, batch=batch, check_items=lambda b: [0, b - 1], seed=batch)
