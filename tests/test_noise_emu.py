"""Lift, centered bits and noise measurement on the device (fhe_poly_lift_dev, fhe_poly_centered_bits_dev,
fhe_bfv_measure_noise_dev): the kernel sources under host emulation at N = 16 ... 4096, against the oracle's
RnsContext.lift / SecretKey.measure_noise and the formula on Python ints.  tests/test_noise_gpu.py runs the same cases
on the MI355X."""
import numpy as np
import pytest

import devop_cases as D
import devop_shapes as S
import encode_cases as E
import noise_cases as N
from helpers import load_engine


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


@pytest.fixture(scope="module")
def sets16():
    return N.lift_sets(16)


def test_lift_every_set(fhe, sets16):
    """L = 1, 2, 3, 4, 5, 9, 16; 36 ... 62-bit moduli; bitlen(q) below, on and above a multiple of 64.  Then every other
    compile-time L (6, 7, 8, 10 ... 15) at N = 256."""
    for moduli in sets16:
        N.case_lift(fhe, False, 16, moduli)
    # L = 6, 7, 8, 10 ... 15 at N = 256: with the sets above, every compile-time instance L = 1 ... 16
    more = N.lift_more_sets()
    assert {len(m) for m in more} | {len(m) for m in sets16} == set(range(1, 17))
    for moduli in more:
        N.case_lift(fhe, False, N.LIFT_MORE_N, moduli)


@pytest.mark.parametrize("n,sizes", [(512, [50, 50, 40]), (512, [60] * 16), (4096, [62, 45, 36])], ids=["512x3", "512x16", "4096x3"])
def test_lift_several_workgroups(fhe, n, sizes):
    N.case_lift(fhe, False, n, N.generate_moduli(sizes, n), batch=1)


def test_lift_generic_instance(fhe):
    """More moduli than the instantiated L: the run-time-L instance."""
    N.case_lift(fhe, False, 16, N.generate_moduli([40] * 17, 16), batch=1)
    N.case_centered_bits(fhe, False, 16, N.generate_moduli([40] * 17, 16))


def test_lift_device_arrays(fhe, sets16):
    N.case_lift(fhe, "abi", 16, sets16[8])
    N.case_centered_bits(fhe, "abi", 16, sets16[8])


def test_centered_bits_every_set(fhe, sets16):
    for moduli in sets16:
        N.case_centered_bits(fhe, False, 16, moduli)
    for moduli in N.lift_more_sets():
        N.case_centered_bits(fhe, False, N.LIFT_MORE_N, moduli)


@pytest.mark.parametrize("sizes", [[62], [44, 42, 42], [60, 60, 60, 60], [52, 51, 51, 51, 51], [57] * 8 + [56], [62] * 16],
                         ids=lambda s: "L%d" % len(s))
def test_centered_bits_workgroup_boundary(fhe, sizes):
    """N = 512: two workgroups per polynomial; the crafted coefficient at 0, 511, 255 and 256."""
    N.case_centered_bits(fhe, False, 512, N.generate_moduli(sizes, 512))


@pytest.mark.parametrize("n,sizes,level", [(16, [62] * 3, 0), (16, [62] * 3, 1), (64, [62, 60, 55], 0), (64, [62, 60, 55], 2),
                                           (512, [50, 50, 40, 36], 1)], ids=["16", "16l1", "64", "64l2", "512l1"])
def test_noise_parity(fhe, n, sizes, level):
    opar, par = E.params(fhe, n, 1153 if n == 16 else E.stock_t(n), moduli_sizes=sizes)
    N.case_noise_parity(fhe, False, opar, par, level=level, batch=2)


def test_noise_parity_f64_rows(fhe):
    """N = 4096, moduli below 2^50: the inverse transform of the phase takes the F64 instance, then the integer one."""
    n = 4096
    opar, par = E.params(fhe, n, E.stock_t(n), moduli_sizes=[50, 50, 40])
    N.case_noise_parity(fhe, False, opar, par, level=0, batch=1)
    fhe.set_f64(False)
    try:
        N.case_null_vs_given(fhe, False, opar, par, level=0, batch=1)
    finally:
        fhe.set_f64(True)


@pytest.mark.parametrize("i", range(3), ids=["general", "class3", "t61"])
def test_null_vs_given(fhe, i):
    opar, par = D.params(fhe, S.roundtrip_shapes()[i])
    N.case_null_vs_given(fhe, False, opar, par, level=0, batch=1)


def test_null_vs_given_small(fhe):
    opar, par = E.params(fhe, 16, 1153, moduli_sizes=[62] * 3)
    N.case_null_vs_given(fhe, False, opar, par, level=0, batch=3)
    N.case_null_vs_given(fhe, "abi", opar, par, level=1, batch=2)


def test_past_decryption_failure(fhe):
    opar, par = E.params(fhe, 16, 1153, moduli_sizes=[62, 50])
    N.case_past_decryption_failure(fhe, False, opar, par)


def test_statuses(fhe):
    opar, par = E.params(fhe, 16, 1153, moduli_sizes=[62] * 3)
    N.case_statuses(fhe, opar, par)
